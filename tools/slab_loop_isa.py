#!/usr/bin/env python3
"""slab_loop_isa.py -- static instruction counts of the slice-ring kernel's consumer loop, from cross-compiled assembly.

    tools/slab_loop_isa.py simian-spacemonkey_amd/csrc 1,1,0,10,2,0,1,1,0,0,0
    tools/slab_loop_isa.py simian-spacemonkey_amd/csrc KEY KEY ... --marks --extra=-fslp-vectorize --keep /tmp/isa --markdown

A key is the template argument list of smk_k_slab<DT, SH, PERM, NW, NL, DIAG, TF, BR, SHD, OCC, NVL> (smk_slab.h), bools as
0 / 1.  The build directory is the one that holds the Makefile and smk_slab.hip.  For each key the tool asks `make -n` for the
command that builds the key's part (smk_slab_part<n>.o), swaps `-c` for `--cuda-device-only -S`, compiles once per part, cuts
the instance out of the assembly and finds the consumer loop:

  * with --marks (the build gets -DSLAB_MARKS) by the marker comments the kernel then emits through SLAB_MARK (`; slab-mark:
    loop head | occupancy bit | blend | loop tail`): the loop is the text from the first to the last marker, widened to whole
    blocks and by the blocks in front that a branch inside goes back to.  The markers are asm statements and hold some code motion back: the marked build is
    within a few instructions of the product's, not identical to it (compare the two `loop` rows); or
  * without, in the product's own code, as the widest span of a backward branch around the `s_sleep` of SLAB_POLL_SLEEP in
    front of the kernel's end (whole loop only, no sub-regions).

It prints, per class, the static counts of the whole loop and of two sub-regions: loop head to the first occupancy-bit marker
(the common path: every sample pays it) and from there to the blend marker (the visible path).  Classes go by mnemonic prefix
alone: v_ vector (of them *_dpp / v_readlane / v_writelane / v_readfirstlane lane moves and v_pk_*_f32 packed fp32), s_ scalar
(of them s_branch / s_cbranch branches and s_waitcnt / s_nop / s_sleep waits), ds_ LDS, global_ global.  A "spill reload" is a
v_readlane from a VGPR that the function also fills with v_writelane: the kernel's source has no v_writelane of its own.

The counts are STATIC and follow the text: run-time variants of a path (uniform branches on launch parameters) all count,
and a block the compiler lays out elsewhere counts where it lies.  Needs hipcc, no GPU.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

CLASSES = ["vector", "lane-move", "packed-fp32", "scalar", "branch", "wait/nop", "LDS", "global", "spill-reload"]


def part_of(k):
    """slab_inst_part of smk_slab.h"""
    dt, shd, occ, nvl = k[0], k[8], k[9], k[10]
    return 5 if nvl else (4 if shd else 3) if occ else (7 if dt == 2 else 2) if shd else 6 if dt == 2 else dt


def symbol_of(k):
    kinds = "iiiiibibbbb"
    return "_Z10smk_k_slabI" + "".join("L%s%dE" % (t, v) for t, v in zip(kinds, k)) + "Ev12RenderParams10SlabParams"


def compile_part(build_dir, part, extra, out):
    target = "smk_slab_part%d.o" % part
    lines = subprocess.check_output(["make", "-C", build_dir, "-n", "-B", target], text=True).splitlines()
    cmd = [l for l in lines if "-DSLAB_PART=%d" % part in l and " -c " in l]
    if not cmd:
        raise SystemExit("make -n %s names no compile command" % target)
    words = cmd[0].split()
    o = words.index("-o")
    words[o + 1] = out
    c = words.index("-c")
    words[c:c + 1] = ["--cuda-device-only", "-S"]
    words += extra
    subprocess.check_call(words, cwd=build_dir, stderr=subprocess.DEVNULL)


def function_text(asm, sym):
    lines = asm.splitlines()
    a = next((i for i, l in enumerate(lines) if l.startswith(sym + ":")), None)
    if a is None:
        raise SystemExit("no instance %s in the assembly (is the key built? smk_slab.h, slab_inst_missing)" % sym)
    b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[a:b]


def resources(asm, sym):
    """the instance's entry of amdhsa.kernels"""
    out = {}
    m = re.search(r"\.name:\s+%s\n" % re.escape(sym), asm)
    if not m:
        return out
    a = asm.rfind("\n  - ", 0, m.start())
    b = asm.find("\n  - ", m.end())
    for key in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        mm = re.search(r"^    \.%s:\s*(\d+)" % key, asm[a:b if b > 0 else len(asm)], re.M)
        if mm:
            out[key] = int(mm.group(1))
    return out


LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")


def find_loop(fn, poll_sleep):
    """(first line, last line, occupancy marker line or None, blend marker line or None) of the consumer loop in fn"""
    labels = {m.group(1): i for i, l in enumerate(fn) for m in [LABEL.match(l)] if m}
    marks = {}
    for i, l in enumerate(fn):
        m = re.match(r"\s*; slab-mark: (.+?)\s*$", l)
        if m:
            marks.setdefault(m.group(1), []).append(i)
    if "loop head" in marks and "loop tail" in marks:
        # the text from the first to the last marker (a rotated loop has its tail in front of its head), widened to whole
        # blocks, then by the blocks in front of it that a branch inside goes back to (the latch's fragments)
        every = [i for v in marks.values() for i in v]
        lo, hi = min(every), max(every)
        start = max((i for i in labels.values() if i <= lo), default=lo)
        end = next((i - 1 for i in range(hi + 1, len(fn)) if LABEL.match(fn[i]) or re.match(r"\s+s_endpgm\b", fn[i])), len(fn) - 1)
        for i in range(start, end + 1):
            m = BRANCH.match(fn[i])
            if m and labels.get(m.group(1), len(fn)) < start:
                start = labels[m.group(1)]
        occ = marks.get("occupancy bit", [None])[0]
        blend = marks.get("blend", [None])[-1]
        return start, end, occ, blend
    # no markers: the widest span of a backward branch around the poll's s_sleep (the poll is an inner loop of the consumer
    # loop, and nothing wider than the consumer loop branches back across it)
    sl = next((i for i, l in enumerate(fn) if re.match(r"\s+s_sleep %d\b" % poll_sleep, l)), None)
    if sl is None:
        raise SystemExit("neither markers nor `s_sleep %d` in the instance" % poll_sleep)
    spans = []
    for i in range(sl, len(fn)):
        if re.match(r"\s+s_endpgm\b", fn[i]):  # (blocks laid out behind the kernel's end branch back from anywhere)
            break
        m = BRANCH.match(fn[i])
        if m and labels.get(m.group(1), len(fn)) < sl:
            spans.append((labels[m.group(1)], i))
    if not spans:
        raise SystemExit("no loop around `s_sleep %d`" % poll_sleep)
    start = min(a for a, _ in spans)
    end = max(b for _, b in spans)
    return start, end, None, None


def count(fn, a, b, spill_vgprs):
    n = dict.fromkeys(CLASSES, 0)
    for l in fn[a:b + 1]:
        l = l.split(";")[0].strip()
        if not l or l.endswith(":") or l.startswith("."):
            continue
        op = l.split()[0]
        if op.startswith("v_"):
            n["vector"] += 1
            if op.endswith("_dpp") or op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
                n["lane-move"] += 1
            if op.startswith("v_pk_") and "_f32" in op:
                n["packed-fp32"] += 1
            m = re.match(r"v_readlane_b32\s+\S+\s+(v\d+),", l)
            if m and m.group(1) in spill_vgprs:
                n["spill-reload"] += 1
        elif op.startswith(("s_branch", "s_cbranch")):
            n["branch"] += 1
        elif op.startswith(("s_waitcnt", "s_nop", "s_sleep")):
            n["wait/nop"] += 1
        elif op.startswith("s_"):
            n["scalar"] += 1
        elif op.startswith("ds_"):
            n["LDS"] += 1
        elif op.startswith("global_"):
            n["global"] += 1
    return n


def report(asm, key, poll_sleep):
    sym = symbol_of(key)
    fn = function_text(asm, sym)
    spill_vgprs = {m.group(1) for l in fn for m in [re.match(r"\s+v_writelane_b32\s+(v\d+),", l)] if m}
    start, end, occ, blend = find_loop(fn, poll_sleep)
    rows = [("loop", count(fn, start, end, spill_vgprs))]
    if occ is not None and blend is not None:
        # (a rotated loop has the end of the turn in front of its head in the text: that part belongs to neither half)
        head = next(i for i, l in enumerate(fn) if "slab-mark: loop head" in l)
        tail = next(i for i, l in enumerate(fn) if "slab-mark: loop tail" in l)
        first = start if head < tail else max(i for i, l in enumerate(fn[:head + 1]) if LABEL.match(l))
        rows.append(("common", count(fn, first, occ - 1, spill_vgprs)))
        rows.append(("visible", count(fn, occ, blend, spill_vgprs)))
    return {"key": key, "symbol": sym, "lines": end - start + 1, "rows": rows, "resources": resources(asm, sym)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("build_dir")
    ap.add_argument("key", nargs="+", help="DT,SH,PERM,NW,NL,DIAG,TF,BR,SHD,OCC,NVL")
    ap.add_argument("--extra", action="append", default=[], help="one more compiler flag (repeatable; a later flag wins over the Makefile's)")
    ap.add_argument("--marks", action="store_true", help="build with -DSLAB_MARKS and split the loop at the markers")
    ap.add_argument("--keep", metavar="DIR", help="keep the parts' assembly here (and reuse what is there)")
    ap.add_argument("--markdown", action="store_true", help="one table row per key and region")
    args = ap.parse_args()
    src = open(os.path.join(args.build_dir, "smk_slab.hip")).read()
    m = re.search(r"SLAB_POLL_SLEEP\s*=\s*(\d+)", src)
    poll_sleep = int(m.group(1)) if m else 2
    keys = []
    for k in args.key:
        v = [int(x) for x in k.split(",")]
        if len(v) != 11:
            ap.error("a key has 11 numbers: " + k)
        keys.append(v)
    tmp = None
    keep = args.keep
    if not keep:
        tmp = tempfile.TemporaryDirectory()
        keep = tmp.name
    os.makedirs(keep, exist_ok=True)
    extra = args.extra + (["-DSLAB_MARKS"] if args.marks else [])
    tag = "".join("_" + re.sub(r"\W", "", e) for e in extra)
    asm_of = {}
    if args.markdown:
        print("| instance | region | " + " | ".join(CLASSES) + " | VGPRs / SGPRs spilled / scratch |")
        print("|---|---|" + "---|" * (len(CLASSES) + 1))
    for k in keys:
        p = part_of(k)
        if p not in asm_of:
            path = os.path.abspath(os.path.join(keep, "smk_slab_part%d%s.s" % (p, tag)))
            if not os.path.exists(path):
                compile_part(args.build_dir, p, extra, path)
            asm_of[p] = open(path).read()
        r = report(asm_of[p], k, poll_sleep)
        res = r["resources"]
        regs = "%s / %s / %s" % (res.get("vgpr_count", "?"), res.get("sgpr_spill_count", "?"), res.get("private_segment_fixed_size", "?"))
        name = "<%s>" % ",".join(str(x) for x in k)
        if args.markdown:
            for region, n in r["rows"]:
                print("| `%s` | %s | %s | %s |" % (name, region, " | ".join(str(n[c]) for c in CLASSES), regs if region == "loop" else ""))
        else:
            print("smk_k_slab%s  part %d  loop of %d lines  VGPRs / SGPRs spilled / scratch bytes: %s" % (name, p, r["lines"], regs))
            print("  %-8s" % "region" + "".join("%13s" % c for c in CLASSES))
            for region, n in r["rows"]:
                print("  %-8s" % region + "".join("%13d" % n[c] for c in CLASSES))
    return 0


if __name__ == "__main__":
    sys.exit(main())
