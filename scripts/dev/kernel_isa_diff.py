#!/usr/bin/env python3
"""Are the kernels of two checkouts the same machine code?  Compiles every HIP source of both trees (libpgo.so's, and the companion library's where the tree has one) for gfx950 to assembly (device side only, the build's own flags, no GPU
needed) and compares, kernel by kernel, the instruction stream and the kernel descriptor (registers, LDS, scratch, kernel-argument size ...).  Comments, debug line directives and
the numbering of local labels are dropped.  Kernels are matched by name: where a change adds a trailing template parameter with a default, DROPPED_DEFAULTS below has to be
edited for that comparison so that an instantiation is matched with the one it was before.

  python scripts/dev/kernel_isa_diff.py <old checkout> <new checkout>

Prints the kernels that differ, that disappeared and that are new; exit status 1 if an existing kernel changed or disappeared."""
import os
import re
import subprocess
import sys
import tempfile

# (pattern, replacement) applied to the demangled names of BOTH trees.  Empty unless the change under comparison added defaulted template parameters to a kernel: list them
# for that comparison, e.g. (r"(mf_spmv_kernel<\w+, \w+), false>", r"\1>") for a third parameter added with the default `false`.
DROPPED_DEFAULTS = []


def assemble(root, out_dir):
    sys.path.insert(0, root)
    try:
        for m in [k for k in sys.modules if k.startswith("solve_keyframe_pose_graph_amd")]:
            del sys.modules[m]
        from solve_keyframe_pose_graph_amd import _build
        flags, sources, hipcc = list(_build.HIP_FLAGS), list(_build.HIP_SOURCES), _build.hipcc_path()
        if hasattr(_build, "SPARSE_SOURCE"):      # libpgo_sparse.so's one translation unit
            sources.append(_build.SPARSE_SOURCE)
    finally:
        sys.path.pop(0)
    procs = []
    for src in sources:
        stem = os.path.splitext(src)[0]
        out = os.path.join(out_dir, stem + ".s")
        cmd = [hipcc] + flags + ["-ffile-prefix-map=%s=." % root, "-cuid=" + stem, '-DPGO_SOURCE_SHA256="-"', "--cuda-device-only", "-S", "-I", os.path.join(root, "include"),
                                 "-I", os.path.join(root, "solve_keyframe_pose_graph_amd", "csrc"), "-x", "hip", os.path.join(root, "solve_keyframe_pose_graph_amd", "csrc", src), "-o", out]
        procs.append((out, subprocess.Popen(cmd, cwd=root, stderr=subprocess.DEVNULL)))
    for out, pr in procs:
        if pr.wait() != 0:
            raise RuntimeError("compiling for %s failed" % out)
    return [out for out, _ in procs]


def kernels(paths):
    """mangled name -> (instruction lines, descriptor lines); the descriptor block sits between the last instruction and the function's end label"""
    body, desc = {}, {}
    for path in paths:
        cur = name = dcur = None
        for line in open(path, errors="replace"):
            m = re.match(r"^(_Z\w+):\s", line)
            if m and cur is None:
                name, cur = m.group(1), []
                continue
            if cur is None:
                continue
            if re.match(r"^\s*\.amdhsa_kernel ", line):
                dcur = []
                continue
            if ".end_amdhsa_kernel" in line:
                desc[name], dcur = dcur, None
                continue
            if line.startswith(".Lfunc_end"):
                body[name], cur = cur, None
                continue
            s = line.split(";")[0].rstrip()
            if s.strip() and not re.match(r"\s*\.(loc|file|cfi)", s):
                (cur if dcur is None else dcur).append(s)
    return {k: (body[k], desc.get(k, [])) for k in body}


def normalised(ks):
    names = list(ks)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    short = {}
    for n, d in zip(names, plain):
        d = re.sub(r"\(.*", "", d.replace("(anonymous namespace)::", "")).replace("void ", "")      # (kernels in an unnamed namespace would all be cut down to "pgo::")
        for pat, rep in DROPPED_DEFAULTS:
            d = re.sub(pat, rep, d)
        short[n] = d
    out = {}
    for n, (body, desc) in ks.items():
        t = "\n".join(body) + "\n--\n" + "\n".join(desc)
        t = re.sub(r"_Z\w+", lambda m: short.get(m.group(0), m.group(0)), t)
        out[short[n]] = re.sub(r"\.L\w+", ".L", t)
    return out


def main():
    old_root, new_root = (os.path.abspath(p) for p in sys.argv[1:3])
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        old, new = normalised(kernels(assemble(old_root, a))), normalised(kernels(assemble(new_root, b)))
    same = sorted(k for k in old if k in new and old[k] == new[k])
    changed = sorted(k for k in old if k in new and old[k] != new[k])
    gone = sorted(k for k in old if k not in new)
    added = sorted(k for k in new if k not in old)
    print("kernels: %d old, %d new; identical instruction stream and descriptor: %d" % (len(old), len(new), len(same)))
    for title, ks in (("changed", changed), ("gone", gone), ("new", added)):
        print("%s: %d" % (title, len(ks)))
        for k in ks:
            print("  " + k)
    return 1 if changed or gone else 0


if __name__ == "__main__":
    sys.exit(main())
