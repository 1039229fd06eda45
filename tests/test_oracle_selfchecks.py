"""Internal-consistency checks of the oracle (the reference has no tests for the xlstm / mamba_ssm boundary,
SURVEY.md 4): step<->parallel, batched<->single env, first-step rule variants, reset semantics, and the
independent pure-torch Mamba implementation that ships with `transformers`."""
import pytest
import torch

from lram_amd import init_state_dict, preset
from lram_amd.config import ModelSpec
from oracle import dt_ref, mamba_ref, xlstm_ref
from tests.helpers import IMAGE_SHAPE_SWEEP, make_inputs, pooled_hw, rel_err


def test_mlstm_step_equals_parallel_form():
    spec = preset("xlstm_c1")
    sd = init_state_dict(spec, seed=2)
    x = torch.randn(3, 12, spec.d_model, generator=torch.Generator().manual_seed(0))
    hs, _ = xlstm_ref.encoder_forward_cached(spec, sd, x, None)
    hp = xlstm_ref.stack_forward_parallel(spec, sd, x)
    # the two forms differ only through eps * exp(m) in the denominator (see oracle/xlstm_ref.py)
    assert rel_err(hs, hp) < 5e-5


@pytest.mark.parametrize("scheme", ["reference", "trained_like"])
def test_mlstm_step_equals_parallel_form_on_the_long_memory_weight_distributions(scheme):
    """The same identity where the recurrence is hard: forget gates of 0.95-0.998 ("reference": a freshly built model) and
    input-gate pre-activations of +-16 with the stabiliser far from 0 ("trained_like"), 96 tokens.  Evaluated in float64 -- the
    regime is ill-conditioned for fp32 (profiles/r06_trained_like_conditioning.txt) and this is a check of the oracle's ALGEBRA
    (stabilised step == row-stabilised parallel form), the thing the GPU parity tests on these distributions lean on."""
    spec = preset("xlstm_c1")
    sd = {k: v.double() for k, v in init_state_dict(spec, seed=2, scheme=scheme).items()}
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        x = torch.randn(2, 96, spec.d_model, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        if scheme == "trained_like":
            x[:, :, 3] *= 30.0
        hs, state = xlstm_ref.encoder_forward_cached(spec, sd, x, None)
        hp = xlstm_ref.stack_forward_parallel(spec, sd, x)
    finally:
        torch.set_default_dtype(prev)
    # (the forms differ by where eps = 1e-6 enters the denominator: measured 5e-8 on "trained_like")
    assert hs.dtype == torch.float64 and rel_err(hs, hp) < 1e-6, rel_err(hs, hp)
    m = state["block_0"]["mlstm_state"][2]
    if scheme == "trained_like":
        assert float(m.abs().max()) > 4.0      # the stabiliser really left the neighbourhood of 0


@pytest.mark.parametrize("name", ["xlstm_tiny", "mamba_tiny"])
def test_batched_equals_single_env(name):
    """Guards cross-env leakage and the sLSTM `n == 0` rule: B envs at once == each env alone."""
    spec = preset(name)
    sd = init_state_dict(spec, seed=3)
    B, steps = 5, 6
    seq = make_inputs(spec, B, steps, seed=77, reset_prob=0.3)
    full = dt_ref.OraclePolicy(spec, sd)
    singles = [dt_ref.OraclePolicy(spec, sd) for _ in range(B)]
    for obs, rtg, rew, mask in seq:
        a = full.step(obs, rtg, rew, mask)
        for b in range(B):
            ab = singles[b].step(obs[b:b + 1], rtg[b:b + 1], rew[b:b + 1], mask[b:b + 1])
            assert float((a[b] - ab[0]).abs().max()) <= 1e-4, (name, b)


def test_slstm_first_step_rule_variants_coincide():
    """per-env all(n == 0) (CPU package path at batch 1) == per-element n == 0 (CUDA kernel) on a trajectory:
    n is zero everywhere before an env's first step and strictly positive afterwards."""
    torch.manual_seed(0)
    B, H = 3, 32
    states = torch.zeros(4, B, H)
    for t in range(6):
        Wx, Ry, b = torch.randn(B, 4, H) * 2, torch.randn(B, 4, H), torch.randn(4, H)
        new = xlstm_ref.slstm_pointwise(Wx, Ry, b, states)
        raw = Wx + Ry + b
        lfm = states[3] + torch.nn.functional.logsigmoid(raw[:, 1])
        m_elem = torch.where(states[2] == 0.0, raw[:, 0], torch.max(raw[:, 0], lfm))
        assert torch.equal(new[3], m_elem)
        assert bool((new[2] > 0).all())
        states = new
        if t == 2:  # reset env 1 mid-trajectory
            states = states.clone()
            states[:, 1] = 0


def test_reset_mask_equals_fresh_policy():
    spec = preset("xlstm_tiny")
    sd = init_state_dict(spec, seed=4)
    B = 3
    seq = make_inputs(spec, B, 4, seed=5, reset_prob=0.0)
    pol = dt_ref.OraclePolicy(spec, sd)
    for obs, rtg, rew, _ in seq:
        pol.step(obs, rtg, rew, None)
    obs, rtg, rew, _ = seq[0]
    a = pol.step(obs, rtg, rew, torch.tensor([0, 1, 0], dtype=torch.uint8))
    fresh = dt_ref.OraclePolicy(spec, sd).step(obs, rtg, rew, None)
    assert torch.equal(a[1], fresh[1]) and not torch.equal(a[0], fresh[0])


def test_state_layout_matches_reference_past_key_values():
    spec = preset("xlstm_16m")
    st = xlstm_ref.zero_state(spec, 2)
    assert st["block_0"]["mlstm_state"][0].shape == (2, 4, 256, 256)
    assert st["block_0"]["mlstm_state"][1].shape == (2, 4, 256, 1)
    assert st["block_0"]["mlstm_state"][2].shape == (2, 4, 1, 1)
    assert st["block_0"]["conv_state"][0].shape == (2, 4, 1024)
    assert st["block_1"]["slstm_state"].shape == (4, 2, 512)
    assert st["block_1"]["conv_state"][0].shape == (2, 4, 512)
    ms = mamba_ref.zero_state(preset("mamba_48m"), 2)
    assert ms[0][0].shape == (2, 1536, 4) and ms[0][1].shape == (2, 1536, 16)


@pytest.mark.parametrize("regime", ["exercise", "trained_like"])
def test_mamba_step_matches_transformers_mixer(regime):
    """T sequential oracle steps == the full-sequence scan of transformers' pure-torch MambaMixer; "trained_like": dt_proj.bias at
    both ends of the initialiser's range (softplus^-1 of 1e-3 / 1e-1), A_log up to log 16 + 2, 40 tokens (the corner
    lram_amd/weights.py::init_state_dict(scheme="trained_like") puts the engine tests in)."""
    tm = pytest.importorskip("transformers.models.mamba.modeling_mamba")
    from transformers import MambaConfig
    D, N, K, R, T, B = 64, 16, 4, 4, (7 if regime == "exercise" else 40), 3
    cfg = MambaConfig(hidden_size=D, state_size=N, conv_kernel=K, expand=2, time_step_rank=R, num_hidden_layers=1,
                      use_bias=False, use_conv_bias=True, vocab_size=8)
    try:
        mixer = tm.MambaMixer(cfg, layer_idx=0).eval()
    except Exception as exc:  # API drift in transformers
        pytest.skip(f"cannot construct MambaMixer: {exc}")
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in mixer.parameters():
            if p.dim() >= 2 and p is not mixer.A_log:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p.shape[-1] ** 0.5))
        mixer.A_log.add_(torch.randn(mixer.A_log.shape, generator=g) * 0.1)
        if regime == "trained_like":
            mixer.A_log.add_(torch.rand(mixer.A_log.shape, generator=g) * 2.0)
            dt = torch.where(torch.rand(mixer.dt_proj.bias.shape, generator=g) < 0.5, torch.tensor(1e-3), torch.tensor(1e-1))
            mixer.dt_proj.bias.copy_(dt + torch.log(-torch.expm1(-dt)))
    x = torch.randn(B, T, D, generator=g)
    with torch.no_grad():
        try:
            y_hf = mixer.slow_forward(x) if hasattr(mixer, "slow_forward") else mixer(x)
        except Exception as exc:
            pytest.skip(f"transformers MambaMixer forward not runnable here: {exc}")
    sd = {"m." + k: v.detach() for k, v in mixer.state_dict().items()}
    conv = torch.zeros(B, 2 * D, K)
    ssm = torch.zeros(B, 2 * D, N)
    outs = []
    for t in range(T):
        o, conv, ssm = mamba_ref.mamba_step(sd, "m.", x[:, t], conv, ssm, R, N)
        outs.append(o)
    assert rel_err(torch.stack(outs, 1), y_hf) < 1e-5


def test_impala_cnn_shapes_and_image_path():
    spec = ModelSpec(backbone="xlstm", d_model=128, n_blocks=1, state_dim=20, act_dim=4)
    sd = init_state_dict(spec, seed=6, with_image_encoder=True)
    assert sd["embed_image.linear.0.weight"].shape == (128, 2048)  # 32 ch x 8 x 8 for 64x64 input
    pol = dt_ref.OraclePolicy(spec, sd)
    img = torch.randint(0, 256, (2, 3, 64, 64), dtype=torch.uint8)
    a = pol.step(img, torch.ones(2), torch.zeros(2), discrete=True)
    assert a.shape == (2, 1) and a.dtype == torch.int64 and int(a.max()) < spec.n_discrete
    # the product's torch image encoder computes the same embedding as the oracle's functional restatement
    from tests.torch_image_encoder import ImageEncoder
    enc = ImageEncoder.from_state_dict(sd, spec.image_shape, spec.d_model)
    ref = dt_ref.impala_cnn(sd, "embed_image.", img.float() / 255.0)
    assert rel_err(enc(img), ref) < 1e-6


def _image_spec(shape):
    return ModelSpec(backbone="xlstm", d_model=128, n_blocks=2, slstm_at=[1], image_shape=shape)


@pytest.mark.parametrize("shape", IMAGE_SHAPE_SWEEP + [(3, 21, 27), (3, 62, 56)], ids=lambda s: "x".join(map(str, s)))
def test_image_layout_pools_height_and_width_separately(shape):
    """reference_layout / init_state_dict / check_state_dict: the linear layer has 32 * h * w columns with the pooled h, w of the
    frame (H and W pooled each on its own, three times), and the first conv takes the frame's channel count."""
    from lram_amd.weights import check_state_dict, reference_layout
    spec = _image_spec(shape)
    h, w = pooled_hw(shape[1], shape[2])
    lay = reference_layout(spec, with_image_encoder=True)
    assert lay["embed_image.linear.0.weight"] == (128, 32 * h * w)
    assert lay["embed_image.cnn.0.conv.weight"] == (16, shape[0], 3, 3)
    sd = init_state_dict(spec, seed=6, with_image_encoder=True)
    assert tuple(sd["embed_image.linear.0.weight"].shape) == (128, 32 * h * w)
    check_state_dict(spec, sd, with_image_encoder=True)


def test_check_state_dict_tells_frame_sizes_apart_by_their_pooled_size():
    """A state dict built for (3, 17, 33) passes the check of its own spec; one built for another pooled size fails it.
    The transposed frame (3, 33, 17) pools to 5 x 3 where (3, 17, 33) pools to 3 x 5: the same 480 columns, so the SHAPES of
    the two state dicts are equal and no shape check can tell them apart (the flatten order differs, the count does not) --
    stated here so that nobody expects otherwise."""
    from lram_amd.weights import check_state_dict, reference_layout
    spec = _image_spec((3, 17, 33))
    check_state_dict(spec, init_state_dict(spec, seed=6, with_image_encoder=True), with_image_encoder=True)
    for other, cols in (((3, 33, 65), 32 * 5 * 9), ((3, 33, 33), 32 * 5 * 5), ((3, 17, 17), 32 * 3 * 3)):
        sd = init_state_dict(_image_spec(other), seed=6, with_image_encoder=True)
        assert sd["embed_image.linear.0.weight"].shape[1] == cols
        with pytest.raises(KeyError, match="embed_image.linear.0.weight"):
            check_state_dict(spec, sd, with_image_encoder=True)
    with pytest.raises(KeyError, match="embed_image.cnn.0.conv.weight"):   # ... and another channel count
        check_state_dict(spec, init_state_dict(_image_spec((1, 17, 33)), seed=6, with_image_encoder=True), with_image_encoder=True)
    assert pooled_hw(33, 17) == (5, 3) and pooled_hw(17, 33) == (3, 5)
    assert reference_layout(_image_spec((3, 33, 17)), True) == reference_layout(spec, True)


@pytest.mark.parametrize("shape", IMAGE_SHAPE_SWEEP, ids=lambda s: "x".join(map(str, s)))
def test_impala_cnn_equals_the_torch_module_at_every_swept_frame_size(shape):
    """The oracle's functional restatement (float32) and tests/torch_image_encoder.ImageEncoder are independent restatements of
    the reference's module: equal to 1e-6 of max |ref| on every frame size of the engine's shape sweep, and float32 stays within
    1e-6 of the float64 evaluation that the GPU tests compare against (measured 2.9e-7 .. 5.0e-7)."""
    from tests.torch_image_encoder import ImageEncoder
    spec = _image_spec(shape)
    sd = init_state_dict(spec, seed=6, with_image_encoder=True)
    img = torch.randint(0, 256, (5, *shape), dtype=torch.uint8, generator=torch.Generator().manual_seed(11))
    ref = dt_ref.impala_cnn(sd, "embed_image.", img.float() / 255.0)
    h, w = pooled_hw(shape[1], shape[2])
    assert ref.shape == (5, 128) and sd["embed_image.linear.0.weight"].shape == (128, 32 * h * w)
    assert float(ref.abs().max()) > 0.0
    assert rel_err(ImageEncoder.from_state_dict(sd, shape, spec.d_model)(img), ref) < 1e-6
    ref64 = dt_ref.impala_cnn({k: v.double() for k, v in sd.items()}, "embed_image.", img.double() / 255.0)
    assert ref64.dtype == torch.float64 and rel_err(ref, ref64) < 1e-6


def test_mlstm_cell_matches_transformers_xlstm_native_step():
    """Independent cross-check of the stabilised mLSTM recurrence (not a parity oracle: the xLSTM-7B variant in
    `transformers.models.xlstm` scales q instead of k and has no conv front end): with the same q, k,
    v and gate pre-activations its `mlstm_recurrent_step_native` gives the same h, m and -- up to the sqrt(DH)
    that moves from k to q -- the same C and n as oracle.xlstm_ref.mlstm_recurrent_step, step after step."""
    import math
    hx = pytest.importorskip("transformers.models.xlstm.modeling_xlstm")
    if not hasattr(hx, "mlstm_recurrent_step_native"):
        pytest.skip("this transformers build routes to the external xlstm package")
    from oracle import xlstm_ref
    g = torch.Generator().manual_seed(5)
    B, NH, DH, S = 3, 4, 32, 12
    c = torch.zeros(B, NH, DH, DH)
    n = torch.zeros(B, NH, DH, 1)
    m = torch.zeros(B, NH, 1, 1)
    c_h, n_h, m_h = torch.zeros(B, NH, DH, DH), torch.zeros(B, NH, DH), torch.zeros(B, NH, 1)
    for t in range(S):
        q, k, v = (torch.randn(B, NH, 1, DH, generator=g) for _ in range(3))
        ig = torch.randn(B, NH, 1, 1, generator=g) * 2.0
        fg = torch.randn(B, NH, 1, 1, generator=g) * 2.0 + 2.0
        h, (c, n, m) = xlstm_ref.mlstm_recurrent_step(c, n, m, q, k, v, ig, fg)
        h_h, (c_h, n_h, m_h) = hx.mlstm_recurrent_step_native(q[:, :, 0], k[:, :, 0], v[:, :, 0], ig[:, :, 0], fg[:, :, 0],
                                                              c_h, n_h, m_h)
        assert torch.allclose(h.squeeze(2), h_h, rtol=1e-5, atol=1e-6), t
        assert torch.allclose(m.view(B, NH, 1), m_h, rtol=0, atol=1e-6), t
    assert torch.allclose(c * math.sqrt(DH), c_h, rtol=1e-5, atol=1e-6)
    assert torch.allclose(n.squeeze(-1) * math.sqrt(DH), n_h, rtol=1e-5, atol=1e-6)


def _stabilised_factors(ig, fg, m0):
    """Per-token factors the kernels share: f_t = exp(logsig(f~_t) + m_{t-1} - m_t), i_t = exp(i~_t - m_t)."""
    import torch.nn.functional as F
    f, i, m = [], [], []
    mp = m0
    for t in range(ig.shape[0]):
        lf = F.logsigmoid(fg[t])
        mn = torch.maximum(lf + mp, ig[t])
        f.append(torch.exp(lf + mp - mn))
        i.append(torch.exp(ig[t] - mn))
        m.append(mn)
        mp = mn
    return torch.stack(f), torch.stack(i), torch.stack(m)


def test_chunkwise_and_lazy_forms_equal_the_recurrent_step():
    """CPU statement of the two algebraic rewrites the HIP kernels use, against the oracle's token-by-token recurrence
    (one head, fp64 to separate algebra from rounding):
      chunkwise (csrc/mlstm_chunk.hip):  H = diag(fcum) Q C_0 + A V,  C_T = fcum_T C_0 + (w K)^T V,
                                         A[t][s] = (f_{s+1}..f_t) i_s (q_t . k_s),  q_t.n_t = fcum_t q_t.n_0 + sum_s A[t][s]
      lazy (csrc/mlstm_lazy.hip):        C_t = g C_base + sum_j c_j k_j v_j^T read through a pending window, folded
                                         every few steps."""
    import math
    from oracle import xlstm_ref
    torch.manual_seed(0)
    DH, T = 16, 23
    dt = torch.float64
    q, k, v = (torch.randn(T, DH, dtype=dt) for _ in range(3))
    ig, fg = torch.randn(T, dtype=dt) * 2, torch.randn(T, dtype=dt) * 2 + 1
    c0, n0, m0 = torch.randn(DH, DH, dtype=dt), torch.randn(DH, dtype=dt), torch.tensor(0.3, dtype=dt)
    # reference: the oracle's recurrent step, token by token
    c, n, m = c0.view(1, 1, DH, DH).clone(), n0.view(1, 1, DH, 1).clone(), m0.view(1, 1, 1, 1).clone()
    h_ref = []
    for t in range(T):
        h, (c, n, m) = xlstm_ref.mlstm_recurrent_step(c, n, m, q[t].view(1, 1, 1, DH), k[t].view(1, 1, 1, DH),
                                                      v[t].view(1, 1, 1, DH), ig[t].view(1, 1, 1, 1), fg[t].view(1, 1, 1, 1))
        h_ref.append(h.view(DH))
    h_ref = torch.stack(h_ref)
    f, i, mt = _stabilised_factors(ig, fg, m0)
    kh = k / math.sqrt(DH)
    # ---- chunkwise form over the whole sequence as one chunk ----
    fcum = torch.cumprod(f, 0)
    A = torch.zeros(T, T, dtype=dt)
    for t in range(T):
        for s in range(t + 1):
            A[t, s] = torch.prod(f[s + 1: t + 1]) * i[s] * (q[t] @ kh[s])
    H = fcum[:, None] * (q @ c0) + A @ v
    den = torch.maximum((fcum * (q @ n0) + A.sum(1)).abs(), torch.exp(-mt)) + 1e-6
    w = torch.stack([torch.prod(f[s + 1:]) * i[s] for s in range(T)])
    C_T = fcum[-1] * c0 + (w[:, None] * kh).T @ v
    assert torch.allclose(H / den[:, None], h_ref, rtol=1e-9, atol=1e-10)
    assert torch.allclose(C_T, c.view(DH, DH), rtol=1e-9, atol=1e-10)
    assert torch.allclose(fcum[-1] * n0 + (w[:, None] * kh).sum(0), n.view(DH), rtol=1e-9, atol=1e-10)
    # ---- lazy form: read-only base + window, folded every 5 tokens; denominators from the eager n recurrence ----
    base, g, win_k, win_v, coef = c0.clone(), torch.tensor(1.0, dtype=dt), [], [], []
    nn_ = n0.clone()
    for t in range(T):
        if t % 5 == 0 and win_k:   # fold
            base = g * base + sum(cj * torch.outer(kj, vj) for cj, kj, vj in zip(coef, win_k, win_v))
            g, win_k, win_v, coef = torch.tensor(1.0, dtype=dt), [], [], []
        g = g * f[t]
        coef = [cj * f[t] for cj in coef] + [i[t]]
        win_k.append(kh[t]), win_v.append(v[t])
        nn_ = f[t] * nn_ + i[t] * kh[t]
        num = g * (q[t] @ base) + sum(cj * (q[t] @ kj) * vj for cj, kj, vj in zip(coef, win_k, win_v))
        d = torch.maximum((q[t] @ nn_).abs(), torch.exp(-mt[t])) + 1e-6
        assert torch.allclose(num / d, h_ref[t], rtol=1e-9, atol=1e-10), t
    final = g * base + sum(cj * torch.outer(kj, vj) for cj, kj, vj in zip(coef, win_k, win_v))
    assert torch.allclose(final, c.view(DH, DH), rtol=1e-9, atol=1e-10)


def test_slstm_cell_equals_the_papers_unstabilised_recurrence():
    """Independent cross-check of the sLSTM cell (the one oracle piece that had none): the xLSTM paper's equations
    (Beck et al. 2024, section 2.2: c_t = f_t c_{t-1} + i_t z_t, n_t = f_t n_{t-1} + i_t, h_t = o_t c_t / n_t with
    i = exp(i~), f = sigmoid(f~), z = tanh(z~), o = sigmoid(o~), pre-activations x~ + R h_{t-1} + b with a block-diagonal
    (per-head) R) written as plain scalar loops in float64, WITHOUT the stabiliser state m -- which by the paper's own
    argument cancels in c / n.  The oracle's stabilised cell (m_t = max(log f + m_{t-1}, i~), the package's first-step
    rule) must give the same h, and its (c, n) must equal the unstabilised ones once multiplied by exp(m).  What this
    cannot pin is the package's storage convention (gate order i, f, z, o; R as [head, in, gate, out]; bias
    [head, gate, out]) -- that is what tests/test_backbone_golden.py is for."""
    import math
    NH, DH, B, T = 2, 4, 3, 9
    H = NH * DH
    g = torch.Generator().manual_seed(77)
    gates = (torch.randn(T, B, 4 * H, generator=g, dtype=torch.float64) * 1.5)
    R = torch.randn(NH, DH, 4, DH, generator=g, dtype=torch.float64) * 0.8
    bias = torch.randn(NH, 4, DH, generator=g, dtype=torch.float64)
    for dtype, tol in ((torch.float64, 1e-11), (torch.float32, 2e-5)):
        states = torch.zeros(4, B, H, dtype=dtype)
        ys = []
        for t in range(T):
            states = xlstm_ref.slstm_cell_step(gates[t].to(dtype), states, R.to(dtype), bias.to(dtype), NH)
            ys.append(states[0].double())
        for b in range(B):
            h, c, n = [0.0] * H, [0.0] * H, [0.0] * H
            for t in range(T):
                h_new, c_new, n_new = [0.0] * H, [0.0] * H, [0.0] * H
                for head in range(NH):
                    for o in range(DH):
                        u = head * DH + o
                        pre = []
                        for gi in range(4):     # gate order of the pre-activation layout: i, f, z, o
                            acc = float(gates[t, b, gi * H + u]) + float(bias[head, gi, o])
                            for i in range(DH):
                                acc += h[head * DH + i] * float(R[head, i, gi, o])
                            pre.append(acc)
                        ig, fg = math.exp(pre[0]), 1.0 / (1.0 + math.exp(-pre[1]))
                        zg, og = math.tanh(pre[2]), 1.0 / (1.0 + math.exp(-pre[3]))
                        c_new[u] = fg * c[u] + ig * zg
                        n_new[u] = fg * n[u] + ig
                        h_new[u] = og * c_new[u] / n_new[u]
                h, c, n = h_new, c_new, n_new
                want = torch.tensor(h, dtype=torch.float64)
                assert float((ys[t][b] - want).abs().max()) <= tol * max(1.0, float(want.abs().max())), (dtype, b, t)
            # stabilised state x exp(m) = unstabilised state
            m = states[3, b].double()
            for got, want in ((states[1, b].double() * torch.exp(m), torch.tensor(c, dtype=torch.float64)),
                              (states[2, b].double() * torch.exp(m), torch.tensor(n, dtype=torch.float64))):
                assert float(((got - want).abs() / (want.abs() + 1e-9)).max()) <= 50 * tol, (dtype, b)
