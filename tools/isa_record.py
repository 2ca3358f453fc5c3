"""Write a profiles/<name>/isa_before_after.json record: the kernels of a library built from the parent
commit beside those of this tree's, and the register / scratch figures of the kernels this tree adds.

    python tools/isa_record.py PARENT.so THIS.so RESOURCE_LOG OUT.json

RESOURCE_LOG is the output of `python -m rl_rocket_amd.build --force --resource-usage` for THIS.so (the
compiler's kernel-resource-usage remarks). The hashes are rl_rocket_amd.build.kernel_isa_hashes'; the
per-translation-unit __hip_cuid_* objects, which are no kernels, are left out (tools/isa_diff.py)."""
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
          "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "LDS Size [bytes/block]": "lds_bytes_per_block"}


def resources(log):
    """{demangled kernel name: figures} from the remarks of a --resource-usage build."""
    out, cur = {}, None
    with open(log) as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+) \[-Rpass-analysis", line)
            if m and cur is not None and m.group(1).strip() in FIELDS:
                cur[FIELDS[m.group(1).strip()]] = int(m.group(2))
    names = sorted(out)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return {p: out[n] for n, p in zip(names, plain.splitlines())}


def main():
    if len(sys.argv) != 5:
        sys.exit(__doc__)
    from isa_diff import kernels
    from rl_rocket_amd.build import ARCH

    before, after, res = kernels(sys.argv[1]), kernels(sys.argv[2]), resources(sys.argv[3])
    added = sorted(k for k in after if k not in before)
    rec = {"what": "build.kernel_isa_hashes of the library built from the parent commit (before) and from this tree "
                   "(after); the per-translation-unit __hip_cuid_* objects, which are no kernels, left out; "
                   "resources: the compiler's kernel-resource-usage remarks for the added kernels",
           "arch": ARCH, "kernels_in_parent": len(before),
           "changed": sum(1 for k, h in before.items() if after.get(k) != h),
           "removed": sorted(k for k in before if k not in after), "added": added,
           "resources": {k: res[k] for k in added}, "before": before, "after": after}
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[4])), exist_ok=True)
    with open(sys.argv[4], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("parent %d kernels, changed %d, removed %d, added %d" % (len(before), rec["changed"], len(rec["removed"]),
                                                                   len(added)))
    return 1 if rec["changed"] or rec["removed"] else 0


if __name__ == "__main__":
    sys.exit(main())
