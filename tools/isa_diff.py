"""Compare the kernels of two builds of librocket_hip.so: the check of a refactor that must not
change a single instruction.

    python tools/isa_diff.py A.so B.so

Runs rl_rocket_amd.build.kernel_isa_hashes (sha256 of each kernel's gfx950 machine code + kernel
descriptor) on both libraries, drops the __hip_cuid_* symbols (their names come from the source
file's path) and prints the kernels only in A, only in B, and those whose hash differs. Exit status
1 if any of the three lists is non-empty. It compares hashes only: to see what differs, disassemble
the kernel from both libraries.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernels(lib):
    from rl_rocket_amd.build import kernel_isa_hashes

    return {k: v for k, v in kernel_isa_hashes(lib).items() if not k.startswith("__hip_cuid_")}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    lists = [("only in A", sorted(set(a) - set(b))), ("only in B", sorted(set(b) - set(a))),
             ("hash differs", sorted(k for k in set(a) & set(b) if a[k] != b[k]))]
    print("A: %d kernels (%s)\nB: %d kernels (%s)" % (len(a), sys.argv[1], len(b), sys.argv[2]))
    for title, names in lists:
        print("%s: %d" % (title, len(names)))
        for k in names:
            print("  " + k)
    return 1 if any(names for _, names in lists) else 0


if __name__ == "__main__":
    sys.exit(main())
