"""The compiler's view of every GEMM kernel instance at two commits, for refactors that must not move the generated code.
  gemm_isa_compare.py dump TREE OUTDIR [SOURCE ...] csrc/gemm_*.hip of a checkout -> OUTDIR/*.s + *.remarks (device only,
                                                    the build's flags + -S -Rpass-analysis=kernel-resource-usage; no GPU needed);
                                                    SOURCE: other file names or globs under csrc (sample_kernels.hip '*_kernels.hip')
  gemm_isa_compare.py compare OUT_A OUT_B REPORT    per instance: resources, K loop (first to last v_mfma), rest of the kernel
  gemm_isa_compare.py resources OUT_A OUT_B REPORT  per instance: resources and a verdict only, for refactors that may move the code
                                                    (changed argument lists) but not what a kernel occupies: no scratch, no spill,
                                                    B's LDS = A's, B's occupancy >= A's; instances are matched by kernel name and
                                                    template arguments, whatever their parameters and whichever file holds them
Comments, debug directives, alignment directives, the __hip_cuid_* symbol and the function number in local labels are stripped
before texts are compared.  (profiles/gemm_refactor_isa.txt and profiles/head_refactor_isa.txt are reports of this script.)"""
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lram_amd.build import FLAGS  # noqa: E402

KEYS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]


def dump(tree, out, patterns=()):
    os.makedirs(out, exist_ok=True)
    csrc = os.path.join(tree, "lram_amd", "csrc")
    sources = sorted({f for pat in (patterns or ["gemm_*.hip"]) for f in glob.glob(os.path.join(csrc, pat))})
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

    def one(src):
        base = os.path.splitext(os.path.basename(src))[0]
        p = subprocess.run([hipcc] + FLAGS + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o",
                                              os.path.join(out, base + ".s")], capture_output=True, text=True)
        open(os.path.join(out, base + ".remarks"), "w").write(p.stderr)
        return base, p.returncode
    with ThreadPoolExecutor(max_workers=6) as pool:
        print(list(pool.map(one, sources)))


def canon(name):
    """Instances are matched by name; template arguments that one side dropped (PF of gemm_f16x2_kernel, ABL of the 8-phase
    kernel, both removed after commit 068f892) are taken out of the other side's name."""
    name = re.sub(r"(gemm_f16x2_kernelILb[01]ELb[01]ELi\d+ELb[01]E)Li[12]E(Lb[01]E)", r"\1\2", name)
    return re.sub(r"(gemm_f16x2_8p_kernelILb[01]ELb[01]E)Li0E(E)", r"\1\2", name)


def kernel_id(name):
    """Kernel name + template arguments of a mangled instance name: what is left once the parameter list is out of it."""
    m = re.search(r"\d+([a-z0-9_]+_kernel)(I(?:L[a-z]n?\d+E)+E)?", name)
    return m.group(1) + (m.group(2) or "") if m else name


def resources(path, canon=canon):
    res, name = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = canon(m.group(1))
            res[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*):\s+(\d+)", line)
        if m and name:
            res[name][m.group(1).strip()] = int(m.group(2))
    return res


def functions(path):
    funcs, name, body = {}, None, []
    for line in open(path):
        line = line.rstrip("\n")
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None and re.match(r"^\.Lfunc_end\d+:", line):
            funcs[canon(name)], name = body, None
        elif name is not None:
            s = line.split(";")[0].rstrip()
            if s.strip() and not re.match(r"^\s*\.(loc|file|cfi_\w+|p2align)\b", s) and "__hip_cuid_" not in s:
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return funcs


def split_loop(body):
    idx = [i for i, l in enumerate(body) if "v_mfma" in l]
    return (body[:idx[0]], body[idx[0]:idx[-1] + 1], body[idx[-1] + 1:]) if idx else (body, [], [])


def renamed_only(x, y):
    """Same instructions in the same order, registers numbered differently?"""
    strip = lambda l: re.sub(r"\b([sv])(\d+|\[\d+:\d+\])", r"\1#", l)  # noqa: E731
    return len(x) == len(y) and all(strip(a) == strip(b) for a, b in zip(x, y))


def compare(pa, nw, report, shown=40):
    out, bad = [__doc__.split("\n")[0], "A = " + pa + ", B = " + nw, ""], 0
    for s in sorted(glob.glob(os.path.join(pa, "*.s"))):
        base = os.path.basename(s)[:-2]
        ra, rb = resources(os.path.join(pa, base + ".remarks")), resources(os.path.join(nw, base + ".remarks"))
        fa, fb = functions(s), functions(os.path.join(nw, base + ".s"))
        out += ["=" * 100, f"{base}.hip: {len(fa)} kernel instances in A, {len(fb)} in B"]
        if set(fa) != set(fb):
            bad += 1
            out.append(f"  INSTANCE SETS DIFFER: only A {sorted(set(fa) - set(fb))}, only B {sorted(set(fb) - set(fa))}")
        for name in sorted(set(fa) & set(fb)):
            a, b = ra.get(name, {}), rb.get(name, {})
            same_res = all(a.get(k) == b.get(k) for k in KEYS)
            parts = list(zip(("before the K loop", "K loop", "after the K loop"), split_loop(fa[name]), split_loop(fb[name])))
            out += ["-" * 100, name, "  A: " + ", ".join(f"{k} {a.get(k)}" for k in KEYS),
                    "  B: " + ", ".join(f"{k} {b.get(k)}" for k in KEYS) + ("   [equal]" if same_res else "   [DIFFERENT]")]
            bad += (not same_res) + (parts[1][1] != parts[1][2])
            for tag, x, y in parts:
                verdict = "identical" if x == y else "same instructions, registers renumbered" if renamed_only(x, y) else "DIFFERENT"
                mf = f", {sum('v_mfma' in l for l in x)} / {sum('v_mfma' in l for l in y)} MFMAs" if tag == "K loop" else ""
                out.append(f"  {tag}: {len(x)} / {len(y)} lines{mf}: {verdict}")
            for tag, x, y in parts:
                if x != y:
                    d = list(difflib.unified_diff(x, y, "A", "B", n=1, lineterm=""))
                    out.append(f"  diff of the part {tag} ({len(d)} lines" + (f", first {shown} shown" if len(d) > shown else "") + "):")
                    out += ["    " + l for l in d[:shown]]
    out += ["=" * 100, f"resource sets or K loops that are not identical: {bad}"]
    open(report, "w").write("\n".join(out) + "\n")
    print(out[-1])


def compare_resources(pa, nw, report):
    keys = KEYS + ["VGPRs Spill", "SGPRs Spill"]
    ra, rb = ({k: v for f in sorted(glob.glob(os.path.join(d, "*.remarks"))) for k, v in resources(f, kernel_id).items()}
              for d in (pa, nw))
    out, bad = ["The compiler's view of every kernel instance of the dumped files at two commits.", "resources only; A = " + os.path.basename(pa.rstrip("/")) + ", B = " + os.path.basename(nw.rstrip("/")), ""], 0
    if set(ra) != set(rb):
        bad += 1
        out.append(f"INSTANCE SETS DIFFER: only A {sorted(set(ra) - set(rb))}, only B {sorted(set(rb) - set(ra))}")
    for name in sorted(set(ra) & set(rb)):
        a, b = ra[name], rb[name]
        why = [f"{k} {b.get(k)}" for k in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill") if b.get(k) != 0]
        if b.get(KEYS[4]) != a.get(KEYS[4]):
            why.append("LDS differs")
        if b.get(KEYS[5], 0) < a.get(KEYS[5], 0):
            why.append("occupancy below A's")
        bad += bool(why)
        out += [name, "  A: " + ", ".join(f"{k} {a.get(k)}" for k in keys), "  B: " + ", ".join(f"{k} {b.get(k)}" for k in keys),
                "  " + ("ok" if not why else "NOT OK: " + "; ".join(why)) +
                ("" if all(a.get(k) == b.get(k) for k in keys) else "   (registers differ)")]
    out += ["", f"{len(set(ra) & set(rb))} instances; not ok: {bad}"]
    open(report, "w").write("\n".join(out) + "\n")
    print(out[-1])


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3], sys.argv[4:])
    elif sys.argv[1] == "resources":
        compare_resources(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        compare(sys.argv[2], sys.argv[3], sys.argv[4])
