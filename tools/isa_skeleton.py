#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly files (hipcc --cuda-device-only -S) of the same translation unit.

    python tools/isa_skeleton.py parent.s this.s

For every kernel: `identical` when the normalised text of its body is the same on both sides, else whether the ordered
"skeleton" - the MFMA, ds_read* / ds_write*, global_load* / global_store* (LDS-DMA included), s_barrier and s_waitcnt
instructions, the last with their counter operands - is the same, with the instruction-count delta (where it is not: whether
the lines that differ are all `s_waitcnt lgkmcnt`, i.e. waits moved or merged, or the order of other instructions, and how
many skeleton lines are involved; `, registers` where next_free_vgpr or accum_offset differ - `, fewer registers` where neither
grew: recorded, inside the gate -, the LDS size differs or the private segment grew);
for every kernel that is not identical `+N -M in MFMA span`: the instructions of the second file between its first and last
v_mfma that a diff of the two bodies (register numbers and labels blanked) does not match to the first file, and the first
file's instructions those diff blocks leave out, nothing netted (+0 -0 = every change lies in the prologue or the epilogue); then the instruction count of
the second file, the registers, the LDS size and the private segment from the kernel descriptor (.amdhsa_*), `parent -> this`
where they differ.
Normalisation: __hip_cuid_<hash> (derived from the source text) and comments. Exit status 1 if a kernel is neither
identical nor skeleton-identical, changes inside its MFMA span, next_free_vgpr / accum_offset or the private segment grew, or the
LDS size differs.
"""
import difflib
import re
import subprocess
import sys

SKELETON = re.compile(r"^(v_mfma_\S+|ds_read\S*|ds_write\S*|global_load\S*|global_store\S*|s_barrier)\b|^(s_waitcnt\b.*)$")
DESC = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def parse(path):
    """-> {kernel: {"body": [instruction lines], "desc": {field: int}}}"""
    kernels, cur, desc_of = {}, None, None
    for raw in open(path):
        line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", raw.split(";")[0]).strip()
        if not line:
            continue
        m = re.match(r"^\.amdhsa_kernel\s+(\S+)", line)
        if m:
            desc_of = m.group(1)
            continue
        if line == ".end_amdhsa_kernel":
            desc_of = None
            continue
        if desc_of is not None:
            m = re.match(r"^\.amdhsa_(\w+)\s+(\S+)", line)
            if m and m.group(1) in DESC and desc_of in kernels:
                kernels[desc_of]["desc"][m.group(1)] = int(m.group(2), 0)
            continue
        m = re.match(r"^(\w+):$", line)
        if m and not line.startswith(".L") and cur is None and m.group(1).startswith("_Z"):
            cur = m.group(1)
            kernels[cur] = {"body": [], "desc": {}}
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            elif not line.startswith(".") or line.startswith(".L"):
                kernels[cur]["body"].append(line)
    return {k: v for k, v in kernels.items() if v["desc"]}


def skeleton(body):
    out = []
    for line in body:
        m = SKELETON.match(line)
        if m:
            out.append(m.group(1) or re.sub(r"\s+", " ", m.group(2)))
    return out


def instructions(body):
    return [l for l in body if not l.endswith(":")]


def changed_in_mfma_span(body_a, body_b):
    """-> (added, dropped): the instructions of body_b between its first and last v_mfma that a diff of the two bodies (register
    numbers and labels blanked) does not match to body_a, and the instructions of body_a that the same diff blocks leave out.
    Nothing is netted: n instructions replaced by n others count +n -n."""
    blank = lambda l: re.sub(r"\b[vsa]\d+\b|\b[vsa]\[\d+:\d+\]|\.LBB\d+_\d+", "R", l)
    a, b = [blank(l) for l in instructions(body_a)], [blank(l) for l in instructions(body_b)]
    mfma = [i for i, l in enumerate(b) if l.startswith("v_mfma")]
    if not mfma:
        return 0, 0
    lo, hi = mfma[0], mfma[-1]
    added = dropped = 0
    for op, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
        if op == "equal":
            continue
        inside = sum(1 for j in range(j1, j2) if lo < j < hi)
        added += inside
        if inside or (j1 == j2 and lo < j1 <= hi):          # the parent's side of a block that touches the span
            dropped += i2 - i1
    return added, dropped


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    names = demangle(sorted(set(a) | set(b)))
    bad = 0
    print(f"{'kernel':<58} {'code':<66} {'insns':>6} {'vgpr':>5} {'accum':>5} {'sgpr':>9} {'LDS':>5} {'private':>8}")
    for k in sorted(set(a) | set(b), key=lambda n: names[n]):
        short = re.sub(r"\(anonymous namespace\)::|^void |\(.*\)$", "", names[k])
        if k not in a or k not in b:
            print(f"{short:<58} only in {'parent' if k in a else 'this tree'}")
            bad += 1
            continue
        ka, kb = a[k], b[k]
        na, nb = len(instructions(ka["body"])), len(instructions(kb["body"]))
        da, db = ka["desc"], kb["desc"]
        ok = True
        if ka["body"] == kb["body"] and da == db:
            code = "identical"
        elif skeleton(ka["body"]) == skeleton(kb["body"]):
            code = f"skeleton-identical, {nb - na:+d} insns"
        else:
            sa, sb = skeleton(ka["body"]), skeleton(kb["body"])
            moved = [l for op, i1, i2, j1, j2 in difflib.SequenceMatcher(None, sa, sb, autojunk=False).get_opcodes() if op != "equal"
                     for l in sa[i1:i2] + sb[j1:j2]]
            what = "lgkmcnt waits" if all(l.startswith("s_waitcnt lgkmcnt") for l in moved) else "order"
            code = f"skeleton differs ({what}: {len(moved)} lines), {nb - na:+d} insns"
            ok = False
        regs = ("next_free_vgpr", "accum_offset")
        if any(db[f] > da[f] for f in regs) or da["group_segment_fixed_size"] != db["group_segment_fixed_size"] or \
                db["private_segment_fixed_size"] > da["private_segment_fixed_size"]:
            code += ", registers"
            ok = False
        elif any(db[f] < da[f] for f in regs):
            code += ", fewer registers"
        if code != "identical":
            span = changed_in_mfma_span(ka["body"], kb["body"])
            code += ", +%d -%d in MFMA span" % span
            ok = ok and span == (0, 0)
        bad += not ok
        col = lambda f: str(da[f]) if da[f] == db[f] else f"{da[f]}->{db[f]}"
        print(f"{short:<58} {code:<66} {nb:>6} {col('next_free_vgpr'):>5} {col('accum_offset'):>5} {col('next_free_sgpr'):>9} "
              f"{col('group_segment_fixed_size'):>5} {col('private_segment_fixed_size'):>8}")
    print(f"{len(set(a) | set(b))} kernels, {bad} outside the gate")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
