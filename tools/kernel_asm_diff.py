"""Kernel-by-kernel comparison of the gfx950 assembly of the GEMM translation units of two source trees (no GPU needed).

    python tools/kernel_asm_diff.py TREE_A TREE_B [--experiments] [--stats REGEX]

Compiles anyv2v_amd/csrc/gemm*.hip and ff_fused.hip of both trees with the Makefile's flags (`--cuda-device-only -S`), cuts the output
into kernels by mangled symbol and compares, per symbol and wherever the kernel lives in either tree: the instruction text (symbol
label .. function end; local label numbers normalised -- they restart per file -- and comments dropped), the `.amdhsa_kernel` descriptor block and the
`amdhsa.kernels` metadata entry.  Prints the symbol count per file and every difference; exit status 1 if there is one.
--experiments: the probe build (-DANYV2V_EXPERIMENTS).  --stats REGEX: also a table (MFMAs, scratch instructions, registers, spills)
of the kernels whose symbol matches, A against B."""
import argparse
import concurrent.futures
import glob
import os
import re
import shutil
import subprocess
import sys

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-Wno-unused-result"]
NO_SLP = ("gemm_ws.hip", "ff_fused.hip")   # as anyv2v_amd/csrc/Makefile


def sources(tree):
    d = os.path.join(tree, "anyv2v_amd", "csrc")
    return sorted(glob.glob(os.path.join(d, "gemm*.hip"))) + [os.path.join(d, "ff_fused.hip")]


def asm(path, experiments):
    extra = (["-fno-slp-vectorize"] if os.path.basename(path) in NO_SLP else []) + (["-DANYV2V_EXPERIMENTS"] if experiments else [])
    out = subprocess.run([HIPCC, *FLAGS, *extra, "--cuda-device-only", "-S", path, "-o", "-"], capture_output=True, text=True)
    if out.returncode != 0:
        sys.exit(f"{path}:\n{out.stderr[-3000:]}")
    return out.stdout


def norm(text):
    """local labels without the per-file function number; comments (they name basic blocks by that number) and blank lines dropped"""
    text = re.sub(r"\.L(BB|func_end|func_begin|tmp|JTI)\d+(_\d+)?", lambda m: ".L" + m.group(1) + (m.group(2) or ""), text)
    lines = (line.split(";", 1)[0].rstrip() for line in text.split("\n"))
    return "\n".join(line for line in lines if line)


def kernels(text):
    """symbol -> dict(body, desc, meta) of one assembly file"""
    k = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        k[m.group(1)] = dict(body=norm(m.group(2)), desc="", meta="")
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        k[m.group(1)]["desc"] = m.group(2)
    meta = text.split("amdhsa.kernels:", 1)[1].split("amdhsa.target:", 1)[0] if "amdhsa.kernels:" in text else ""
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:
        k[re.search(r"\.name:\s+(\S+)", entry).group(1)]["meta"] = entry
    return k


def tree_kernels(tree, experiments):
    srcs = sources(tree)
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        texts = list(ex.map(lambda p: asm(p, experiments), srcs))
    per_file = {os.path.basename(p): kernels(t) for p, t in zip(srcs, texts)}
    merged = {}
    for f, ks in per_file.items():
        for sym, v in ks.items():
            assert sym not in merged, f"{sym} is defined in {merged[sym]['file']} and {f}"
            merged[sym] = dict(v, file=f)
    return per_file, merged


def stat(k):
    g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", k["meta"]).group(1))
    return dict(mfma=len(re.findall(r"^\s*v_mfma", k["body"], re.M)), scratch=len(re.findall(r"^\s*scratch_", k["body"], re.M)),
                vgpr=g("vgpr_count"), agpr=g("agpr_count"), private=g("private_segment_fixed_size"), spill=g("vgpr_spill_count"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--experiments", action="store_true")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    (fa, ka), (fb, kb) = tree_kernels(a.tree_a, a.experiments), tree_kernels(a.tree_b, a.experiments)
    for name, f in (("A", fa), ("B", fb)):
        print(f"{name}: " + ", ".join(f"{n} {len(k)}" for n, k in f.items()) + f" -- {sum(len(k) for k in f.values())} kernels")
    bad = 0
    for sym in sorted(set(ka) | set(kb)):
        if sym not in ka or sym not in kb:
            print(f"only in {'A' if sym in ka else 'B'}: {sym}")
            bad += 1
            continue
        diff = [what for what in ("body", "desc", "meta") if ka[sym][what] != kb[sym][what]]
        if diff:
            print(f"differs ({', '.join(diff)}): {sym}  [{ka[sym]['file']} -> {kb[sym]['file']}]")
            bad += 1
    print(f"{len(set(ka) & set(kb))} common symbols, {bad} with a difference")
    if a.stats:
        for sym in sorted(s for s in set(ka) & set(kb) if re.search(a.stats, s)):
            sa, sb = stat(ka[sym]), stat(kb[sym])
            print(sym + "\n    " + " | ".join(f"{key} {sa[key]} -> {sb[key]}" for key in sa))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
