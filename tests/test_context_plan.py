"""Stored contexts of per-env length, the host side (no GPU): the chunk plan (lram_context_plan and its Python mirror
engine.context_plan), the length rules (engine.check_context_lengths) and the three entries in header and ctypes table."""
import ctypes
import os
import random
import re

import pytest
import torch

from lram_amd import engine
from lram_amd.engine import check_context_lengths, context_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lram_hip.h")


def _cases(n=400, seed=7):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        L = rnd.randint(1, 70)
        cap = rnd.choice([4, 16, 21])
        B = rnd.randint(1, 8)
        kind = rnd.random()
        if kind < 0.15:
            lengths = [L] * B
        elif kind < 0.3:     # few distinct lengths, some slots without a context
            pool = [rnd.randint(0, L) for _ in range(2)] + [0, L]
            lengths = [rnd.choice(pool) for _ in range(B)]
        else:
            lengths = [rnd.randint(0, L) for _ in range(B)]
        if not any(lengths):
            lengths[rnd.randrange(B)] = rnd.randint(1, L)
        out.append((L, cap, lengths))
    return out


def _dense_stride(L, cap):
    return list(range(0, L, cap))


def test_plan_properties_over_random_lengths():
    n_dense = n_late = 0
    for L, cap, lengths in _cases():
        plan = context_plan(L, lengths, cap)
        what = (L, cap, lengths, plan)
        s = sorted({L - n for n in lengths if n > 0})
        assert plan == sorted(set(plan)), what                            # ascending, no chunk twice
        assert plan[0] == s[0], what                                      # nothing runs ahead of the first context
        assert set(s) <= set(plan), what                                  # every env starts on a chunk boundary
        ends = plan[1:] + [L]
        assert all(0 < e - b <= cap for b, e in zip(plan, ends)), what    # the chunks tile [first, L), none above cap
        assert all(0 <= t < L for t in plan), what
        if all(n == L for n in lengths):
            assert plan == _dense_stride(L, cap), what
            n_dense += 1
        n_late += plan[0] > 0
        # between two forced boundaries: equal chunks, as few as the cap allows
        bounds = s + [L]
        if s != [0]:
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                inside = [t for t in plan if lo <= t < hi]
                n = -(-(hi - lo) // cap)
                assert len(inside) == n and inside == list(range(lo, hi, -(-(hi - lo) // n))), what
    assert n_dense >= 20 and n_late >= 50    # the sweep reaches both ends


def test_plan_with_only_full_and_empty_slots_is_the_dense_one():
    for L, cap in ((9, 4), (47, 16), (1, 4), (64, 21)):
        assert context_plan(L, [L, 0, L], cap) == _dense_stride(L, cap)
    # the shape of the GPU tests: 47 timesteps, chunks of at most 16
    assert context_plan(47, [47, 47, 30, 30, 9, 1], 16) == [0, 9, 17, 28, 38, 46]
    assert context_plan(12, [0, 12, 0, 5], 12) == [0, 7]
    assert context_plan(5, [1, 0], 4) == [4]


def _c_plan(lib, L, cap, lengths, max_chunks=None):
    n = ctypes.c_int32(-1)
    room = L if max_chunks is None else max_chunks
    out = (ctypes.c_int32 * max(1, room))()
    arr = (ctypes.c_int32 * len(lengths))(*lengths)
    rc = lib.lram_context_plan(L, cap, arr, len(lengths), out, room, ctypes.byref(n))
    return rc, list(out[: max(0, min(n.value, room))]), n.value


def test_c_plan_equals_the_python_mirror(hip_lib):
    for L, cap, lengths in _cases(300, seed=11):
        rc, plan, n = _c_plan(hip_lib, L, cap, lengths)
        assert rc == 0, hip_lib.lram_last_error()
        assert n == len(plan) and plan == context_plan(L, lengths, cap), (L, cap, lengths)
    # refusals name the cause; a buffer that is too small still reports the chunk count
    rc, _, n = _c_plan(hip_lib, 47, 16, [47, 30, 9, 1], max_chunks=2)
    assert rc != 0 and n == 6 and b"6 chunks" in hip_lib.lram_last_error()
    for lengths, needle in (([3, 48], b"outside 0 .. timesteps"), ([-1, 4], b"outside 0 .. timesteps"), ([0, 0], b"every length is 0")):
        rc, _, _ = _c_plan(hip_lib, 47, 16, lengths)
        assert rc != 0 and needle in hip_lib.lram_last_error(), hip_lib.lram_last_error()
    rc, _, _ = _c_plan(hip_lib, 47, 0, [47])
    assert rc != 0
    # (a call that succeeds clears the thread's error text again)
    assert _c_plan(hip_lib, 47, 16, [47])[:2] == (0, [0, 16, 32]) and hip_lib.lram_last_error() == b""


def test_length_rules():
    assert check_context_lengths([3, 0, 5], 3, 5) == [3, 0, 5]
    assert check_context_lengths(torch.tensor([3, 0, 5]), 3, 5) == [3, 0, 5]
    assert check_context_lengths(torch.tensor([5, 5], dtype=torch.int32), 2, 5) == [5, 5]
    import numpy as np
    assert check_context_lengths(np.array([1, 2]), 2, 5) == [1, 2]
    for bad, needle in (([3, -1, 5], "outside 0 .. 5"), ([3, 6, 5], "outside 0 .. 5"), ([0, 0, 0], "every length is 0"),
                        ([3, 4], "expected 3 entries"), ([1, 2, 3, 4], "expected 3 entries"),
                        (torch.tensor([1.0, 2.0, 3.0]), "integer"), ([1.5, 2, 3], "integer"), ([True, 2, 3], "integer"),
                        (torch.tensor([True, False, True]), "integer")):
        with pytest.raises(ValueError) as err:
            check_context_lengths(bad, 3, 5)
        assert needle in str(err.value), (bad, str(err.value))
    with pytest.raises(ValueError):
        context_plan(5, [1, 2], 0)


def test_header_and_ctypes_table_hold_the_three_entries():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, n_args in (("lram_prefill_ragged", 12), ("lram_score_ragged", 19), ("lram_context_plan", 7)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/lram_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        assert name in engine._SYMBOLS and len(engine._SYMBOLS[name][1]) == n_args, name
    # the ragged entries take the dense entries' arguments with host_lengths behind `timesteps`
    for dense, ragged in (("lram_prefill", "lram_prefill_ragged"), ("lram_score", "lram_score_ragged")):
        d, r = engine._SYMBOLS[dense][1], engine._SYMBOLS[ragged][1]
        assert r[:6] == d[:6] and r[7:] == d[6:] and r[6] is ctypes.c_void_p, ragged
