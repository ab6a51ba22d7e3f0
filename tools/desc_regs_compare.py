#!/usr/bin/env python3
"""Resource class of the descriptor family's kernels (bp_*, dtrain*, cf_*, ct_*, ang_*, at_*, cmt_*, committee_*) in two builds of libhtf_amd.so,
read from the code-object notes (no GPU): VGPRs, the waves per SIMD they allow, SGPRs, scratch, VGPR and SGPR spills and
static LDS.  Prints one markdown row per kernel whose figures differ (--all: every kernel) and a summary; exits 1 if a kernel
of the second library has scratch or VGPR spills, spills more SGPRs (to VGPR lanes) than in the first, allows fewer waves per
SIMD, or is missing from either.

Waves per SIMD are those the registers allow: min(8, 512 // alloc), alloc = VGPRs rounded up to the granule of 8.  That covers
the sweeps' __launch_bounds__(256, 1) -- a form above 256 registers gets 1 -- but not LDS: the family's LDS is dynamic (the
notes' static size is 0 for every kernel) and a function of the call's widths alone, which no change to a kernel body moves.
--family REGEX compares another family: the kernels whose name (without ``htf::``) the expression matches at its start, e.g. the
pair path's 'fused_|eval_pair|pair_mlp|mlp_grad|mlp_re|topk_|train_|build_pair|cf_pair|nlist_rinv|check_nlist|reduce_|bias_combine|optimizer_'.
usage: tools/desc_regs_compare.py BEFORE.so AFTER.so [--all] [--family REGEX]"""
import argparse
import pathlib
import re
import struct
import subprocess
import sys
import tempfile

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
FAMILY = "bp_|dtrain|cf_|ct_|ang_|at_|cmt_|committee_"
KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")


def waves(vgprs):
    return min(8, 512 // (-(-vgprs // 8) * 8))


def family(lib, regex=FAMILY):
    """{kernel: {key: value}} of the family's kernels in the gfx950 code objects bundled into lib (the walk of
    tests/test_codeobj.py, with the keys wanted here)."""
    data = pathlib.Path(lib).read_bytes()
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data):
            p = m.start()
            (n,) = struct.unpack_from("<Q", data, p + 24)
            o = p + 32
            for _ in range(n):
                off, size, tl = struct.unpack_from("<QQQ", data, o)
                o += 24
                triple = data[o:o + tl].decode()
                o += tl
                if "gfx950" not in triple or size == 0:
                    continue
                f = pathlib.Path(tmp) / "co.elf"
                f.write_bytes(data[p + off:p + off + size])
                txt = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
                for blk in txt.split("  - .agpr_count:")[1:]:
                    name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                    meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in KEYS}
    names = sorted(meta)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    out = {}
    want = re.compile(r"^htf::(%s)" % regex)
    for n, d in zip(names, dem):
        short = d.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
        if want.match(short):
            out[short[5:]] = meta[n]
    return out


def main():
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--family", default=FAMILY, metavar="REGEX")
    a = ap.parse_args()
    show_all = a.all
    before, after = family(a.before, a.family), family(a.after, a.family)
    bad = sorted(set(before) ^ set(after))
    same = 0
    print("| kernel | VGPRs | waves/SIMD | SGPRs | scratch + VGPR spills | SGPR spills | LDS |")
    print("|---|---|---|---|---|---|---|")
    for k in sorted(after):
        if k not in before:
            continue
        b, a = before[k], after[k]
        dirty = a["private_segment_fixed_size"] or a["vgpr_spill_count"] or a["sgpr_spill_count"] > b["sgpr_spill_count"]
        if dirty or waves(a["vgpr_count"]) < waves(b["vgpr_count"]):
            bad.append(k)
        same += a == b
        if a == b and not show_all:
            continue
        print("| %s | %d -> %d | %d -> %d | %d -> %d | %d -> %d | %d -> %d | %d -> %d |" % (
            k, b["vgpr_count"], a["vgpr_count"], waves(b["vgpr_count"]), waves(a["vgpr_count"]), b["sgpr_count"], a["sgpr_count"],
            b["private_segment_fixed_size"] + b["vgpr_spill_count"], a["private_segment_fixed_size"] + a["vgpr_spill_count"],
            b["sgpr_spill_count"], a["sgpr_spill_count"], b["group_segment_fixed_size"], a["group_segment_fixed_size"]))
    print("\n%d kernels, %d with every figure unchanged; %d fail: %s" % (len(after), same, len(bad), ", ".join(bad) or "-"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
