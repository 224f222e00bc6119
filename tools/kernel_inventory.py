#!/usr/bin/env python3
"""kernel_inventory.py -- the register and memory figures of every gfx950 kernel in a build, from the code objects' metadata.

    tools/kernel_inventory.py libsmk_hip.so -o new.json          # or object files: csrc/*.o
    tools/kernel_inventory.py old.json new.json                  # which kernels were added, removed, changed
    tools/kernel_inventory.py old/libsmk_hip.so libsmk_hip.so    # the same, straight from two builds

Each input is a shared library, object files (several, joined by commas, count as one build) or a JSON file this tool wrote.
From each binary the .hip_fatbin section is dumped (llvm-objcopy), its offload bundles are unbundled for the target
(clang-offload-bundler) and the AMDGPU metadata note is read (llvm-readelf --notes).  Metadata only: no disassembly.
Output: {kernel name: {vgprs, sgprs, agprs, private_segment, group_segment, vgpr_spills, sgpr_spills}}.  With two inputs
the exit status is 1 where they differ.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = {"vgpr_count": "vgprs", "sgpr_count": "sgprs", "agpr_count": "agprs", "private_segment_fixed_size": "private_segment",
          "group_segment_fixed_size": "group_segment", "vgpr_spill_count": "vgpr_spills", "sgpr_spill_count": "sgpr_spills"}
# a kernel's own keys sit four columns in ("  - .agpr_count: 0" opens it); its arguments' keys sit deeper
KEY = re.compile(r"^(  - |    )\.(\w+):\s*(\S+)\s*$")


def llvm_tool(name):
    for d in [os.environ.get("LLVM_BIN", ""), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")]:
        if d and os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return name


def notes_of(binary, tmp):
    """the metadata notes of every gfx950 code object bundled in `binary`, as text"""
    fatbin = os.path.join(tmp, "fatbin")
    subprocess.check_call([llvm_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fatbin, binary, os.path.join(tmp, "copy")])
    data = open(fatbin, "rb").read()
    starts = [m.start() for m in re.finditer(MAGIC, data)]  # (a linked library holds one bundle per translation unit)
    if not starts:
        raise SystemExit("%s: no offload bundle in .hip_fatbin" % binary)
    for a, b in zip(starts, starts[1:] + [len(data)]):
        bundle, elf = os.path.join(tmp, "bundle"), os.path.join(tmp, "code.elf")
        open(bundle, "wb").write(data[a:b])
        subprocess.check_call([llvm_tool("clang-offload-bundler"), "--type=o", "--unbundle", "--targets=" + TARGET, "--input=" + bundle,
                               "--output=" + elf])
        if os.path.getsize(elf):
            yield subprocess.check_output([llvm_tool("llvm-readelf"), "--notes", elf], text=True)


def inventory(spec):
    if spec.endswith(".json"):
        return json.load(open(spec))
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp:
        for binary in spec.split(","):
            for text in notes_of(binary, tmp):
                cur = None
                for line in text.splitlines():
                    m = KEY.match(line)
                    if line.startswith("  - "):  # the next kernel of amdhsa.kernels
                        cur = {}
                    if not m or cur is None:
                        continue
                    if m.group(2) == "name":
                        if m.group(3) in kernels:
                            raise SystemExit("%s: kernel %s appears twice" % (spec, m.group(3)))
                        kernels[m.group(3)] = cur
                    elif m.group(2) in FIELDS:
                        cur[FIELDS[m.group(2)]] = int(m.group(3))
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("build", nargs="+", help="one build to list, or two to compare")
    ap.add_argument("-o", "--output", action="append", default=[], help="write a build's inventory here as JSON (once per build, in order)")
    args = ap.parse_args()
    if len(args.build) > 2:
        ap.error("one build or two")
    inv = [inventory(b) for b in args.build]
    for path, k in zip(args.output, inv):
        json.dump(k, open(path, "w"), indent=0, sort_keys=True)
    if len(inv) == 1:
        if not args.output:
            json.dump(inv[0], sys.stdout, indent=0, sort_keys=True)
        print("%d kernels" % len(inv[0]), file=sys.stderr)
        return 0
    old, new = inv
    added, removed = sorted(set(new) - set(old)), sorted(set(old) - set(new))
    changed = sorted(n for n in set(old) & set(new) if old[n] != new[n])
    for n in added:
        print("added   %s %s" % (n, json.dumps(new[n], sort_keys=True)))
    for n in removed:
        print("removed %s %s" % (n, json.dumps(old[n], sort_keys=True)))
    for n in changed:
        print("changed %s %s" % (n, ", ".join("%s %s -> %s" % (f, old[n].get(f), new[n].get(f)) for f in FIELDS.values() if old[n].get(f) != new[n].get(f))))
    print("%d kernels before, %d after: %d added, %d removed, %d changed" % (len(old), len(new), len(added), len(removed), len(changed)))
    return 1 if added or removed or changed else 0


if __name__ == "__main__":
    sys.exit(main())
