"""In-tree native builds: libpgo.so (HIP, gfx950) and libpgo_graphgen.so (host).  No JIT cache: the built
.so files live next to the sources so that they travel to the GPU box with the repo snapshot."""
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
LIBPGO = os.path.join(_HERE, "libpgo.so")
LIBGEN = os.path.join(_HERE, "libpgo_graphgen.so")

HIP_SOURCES = ["pgo_kernels.hip", "pgo_solver.hip", "pgo_graph.hip", "pgo_shard.hip", "pgo_measure.hip", "pgo_pcg.hip", "pgo_multigrid.hip", "pgo_comm.hip", "pgo_dense.hip"]
HIP_HEADERS = ["pgo_handle.hpp", "pgo_internal.hpp", "pgo_lm.hpp", "pgo_mg_cycle.hpp", "pgo_device_math.hpp", "pgo_mg_kernels.hpp", "pgo_mg_host.hpp", "pgo_comm.hpp", "pgo_dense_math.hpp", "pgo_tile_ops.hpp", "pgo_pcg_ops.hpp"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def hipcc_path():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: libpgo cannot be built (there is no CPU fallback)")


def build_graphgen(force=False):
    src = os.path.join(CSRC, "pgo_graphgen.cpp")
    if force or _stale(LIBGEN, [src, os.path.join(INCLUDE, "pgo_graphgen.h")]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", INCLUDE, "-o", LIBGEN, src])
    return LIBGEN


HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on"]
_ROOT = os.path.dirname(_HERE)
OBJ_DIR = os.path.join(_ROOT, "build", "obj")


def source_tree_hash(extra_flags=()):
    """sha256 over the sources libpgo.so is built from (names relative to the repo root, then contents, in a fixed order) and the compiler flags: what pgo_build_info()
    reports for a library built by build_libpgo(), recomputable from a checkout (bench.py prints both)."""
    import hashlib
    h = hashlib.sha256()
    files = [os.path.join(CSRC, f) for f in HIP_SOURCES + HIP_HEADERS] + [os.path.join(INCLUDE, "pgo.h")]
    for f in files:
        h.update(os.path.relpath(f, _ROOT).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(HIP_FLAGS + list(extra_flags)).encode())
    return h.hexdigest()


def compile_libpgo(target, extra_flags=(), verbose=False, obj_dir=None):
    """Reproducible build: every translation unit to an object of its own with a FIXED compilation-unit id (clang otherwise draws a random one per run: two builds of the
    same sources differed in a few hundred bytes), source paths mapped relative to the repo root, no linker build-id — the same sources and flags give the same bytes whatever
    the checkout's path.  The objects are compiled side by side."""
    obj_dir = obj_dir or OBJ_DIR
    os.makedirs(obj_dir, exist_ok=True)
    sha = source_tree_hash(extra_flags)
    procs, objs = [], []
    for src in HIP_SOURCES:
        stem = os.path.splitext(src)[0]
        obj = os.path.join(obj_dir, stem + ".o")
        cmd = [hipcc_path()] + HIP_FLAGS + list(extra_flags) + ["-ffile-prefix-map=%s=." % _ROOT, "-cuid=" + stem, '-DPGO_SOURCE_SHA256="%s"' % sha,
                                                                "-I", INCLUDE, "-I", CSRC, "-x", "hip", "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
        procs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    subprocess.check_call([hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", target, "-ldl", "-Wl,--build-id=none"])
    return target


def build_libpgo(force=False, verbose=False):
    srcs = [os.path.join(CSRC, s) for s in HIP_SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in HIP_HEADERS] + [os.path.join(INCLUDE, "pgo.h")]
    if force or _stale(LIBPGO, deps):
        compile_libpgo(LIBPGO, verbose=verbose)
    return LIBPGO


LIBSPARSE = os.path.join(_HERE, "libpgo_sparse.so")
SPARSE_SOURCE = "pgo_sparse.hip"
SPARSE_HEADERS = ["pgo_sparse_kernels.hpp", "pgo_sparse_blocks.hpp", "pgo_sparse_math.hpp", "pgo_dense_math.hpp", "pgo_sparse_lm.hpp", "pgo_sparse_lm_math.hpp", "pgo_sparse_graph.hpp", "pgo_sparse_graph_math.hpp", "pgo_sparse_yaw.hpp", "pgo_sparse_yaw_math.hpp"]
# headers of libpgo.so that the companion includes unchanged (the LM controller: one copy of Ceres' rules; the fp64 MFMA tile bodies: one copy of the operand maps and
# the summation order; the closed forms of the cost functors); they belong to HIP_HEADERS, here they are only dependencies
SPARSE_SHARED_HEADERS = ["pgo_lm.hpp", "pgo_tile_ops.hpp", "pgo_device_math.hpp"]
SPARSE_OBJ_DIR = os.path.join(_ROOT, "build", "obj_sparse")
# every symbol include/pgo_sparse.h declares
SPARSE_EXPORTS = ["pgo_sparse_spd_solve", "pgo_sparse_chol_create", "pgo_sparse_chol_destroy", "pgo_sparse_chol_info", "pgo_sparse_chol_factor", "pgo_sparse_chol_solve",
                  "pgo_sparse_chol_inverse_blocks", "pgo_sparse_chol_selected_inverse", "pgo_sparse_chol_selected_info", "pgo_sparse_chol_selected_blocks", "pgo_sparse_chol_inverse_columns", "pgo_sparse_chol_columns_info", "pgo_sparse_chol_set_workspace_limit", "pgo_sparse_reduce_normal_blocks", "pgo_sparse_chol_last_ms", "pgo_sparse_strerror", "pgo_sparse_last_error",
                  "pgo_sparse_lm_create", "pgo_sparse_lm_destroy", "pgo_sparse_lm_set_scale", "pgo_sparse_lm_step", "pgo_sparse_lm_last_times", "pgo_sparse_lm_solve",
                  "pgo_sparse_graph_create", "pgo_sparse_graph_destroy", "pgo_sparse_graph_add_relpose_edges", "pgo_sparse_graph_add_switchable_edges", "pgo_sparse_graph_set_node_regularizers",
                  "pgo_sparse_graph_set_nodes_constant", "pgo_sparse_graph_finalize", "pgo_sparse_graph_evaluate", "pgo_sparse_graph_normal_blocks", "pgo_sparse_graph_jacobian_blocks",
                  "pgo_sparse_graph_manifold_plus", "pgo_sparse_graph_lm_callbacks", "pgo_sparse_graph_edge_lists", "pgo_sparse_graph_last_times",
                  "pgo_sparse_yaw_graph_create", "pgo_sparse_yaw_graph_destroy", "pgo_sparse_yaw_graph_add_edges", "pgo_sparse_yaw_graph_set_nodes_constant", "pgo_sparse_yaw_graph_finalize",
                  "pgo_sparse_yaw_graph_evaluate", "pgo_sparse_yaw_graph_normal_blocks", "pgo_sparse_yaw_graph_jacobian_blocks", "pgo_sparse_yaw_graph_manifold_plus",
                  "pgo_sparse_yaw_graph_lm_callbacks", "pgo_sparse_yaw_graph_edge_lists", "pgo_sparse_yaw_graph_last_times"]


def compile_libpgo_sparse(target, verbose=False, obj_dir=None):
    """libpgo_sparse.so (csrc/pgo_sparse.hip, include/pgo_sparse.h): the tile-sparse Cholesky companion library.  One translation unit, compile_libpgo's reproducibility
    flags, objects in a directory of their own; it does not link libpgo.so.  verbose: the kernels' resource usage on stderr."""
    obj_dir = obj_dir or SPARSE_OBJ_DIR
    os.makedirs(obj_dir, exist_ok=True)
    stem = os.path.splitext(SPARSE_SOURCE)[0]
    obj = os.path.join(obj_dir, stem + ".o")
    cmd = [hipcc_path()] + HIP_FLAGS + ["-ffile-prefix-map=%s=." % _ROOT, "-cuid=" + stem, "-I", INCLUDE, "-I", CSRC, "-x", "hip", "-c", os.path.join(CSRC, SPARSE_SOURCE), "-o", obj]
    if verbose:
        cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
    subprocess.check_call(cmd)
    subprocess.check_call([hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", obj, "-o", target, "-Wl,--build-id=none"])
    return target


def build_libpgo_sparse(force=False, verbose=False):
    deps = [os.path.join(CSRC, f) for f in [SPARSE_SOURCE] + SPARSE_HEADERS + SPARSE_SHARED_HEADERS] + [os.path.join(INCLUDE, "pgo_sparse.h"), os.path.join(INCLUDE, "pgo.h")]
    if force or _stale(LIBSPARSE, deps):
        compile_libpgo_sparse(LIBSPARSE, verbose=verbose)
    return LIBSPARSE


LIBHOST = os.path.join(_HERE, "libpgo_host.so")


def build_host(force=False):
    """C++ host side above the C-ABI (csrc/host/PoseGraphSLAM.*): plain g++, links libpgo.so next to it."""
    build_libpgo(force)
    srcs = [os.path.join(CSRC, "host", "PoseGraphSLAM.cpp"), os.path.join(CSRC, "host", "GraphFormats.cpp")]
    deps = srcs + [os.path.join(CSRC, "host", "PoseGraphSLAM.hpp"), os.path.join(CSRC, "host", "GraphFormats.hpp"), os.path.join(CSRC, "pgo_device_math.hpp"), os.path.join(INCLUDE, "pgo.h"), LIBPGO]
    if force or _stale(LIBHOST, deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", INCLUDE, "-I", CSRC, "-o", LIBHOST] + srcs +
                              ["-L", _HERE, "-l:libpgo.so", "-Wl,-rpath,$ORIGIN"])
    return LIBHOST


EXAMPLE_REPLAY = os.path.join(os.path.dirname(_HERE), "examples", "replay_session")


def build_examples(force=False):
    """examples/replay_session.cpp: the C++ host classes used directly (what a maintainer's code looks like)."""
    build_host(force)
    src = EXAMPLE_REPLAY + ".cpp"
    if force or _stale(EXAMPLE_REPLAY, [src, LIBHOST, os.path.join(CSRC, "host", "PoseGraphSLAM.hpp"), os.path.join(CSRC, "host", "GraphFormats.hpp")]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", INCLUDE, "-I", CSRC, "-o", EXAMPLE_REPLAY, src, "-L", _HERE, "-l:libpgo_host.so", "-l:libpgo.so",
                               "-Wl,-rpath," + _HERE])
    return EXAMPLE_REPLAY


EXAMPLE_RANKS = os.path.join(os.path.dirname(_HERE), "examples", "ranks_in_process")


def build_example_ranks(force=False):
    """examples/ranks_in_process.cpp: N ranks of the sharded solver from one C++ process through the C-ABI alone (in-process communicator)."""
    build_libpgo(force); build_graphgen(force)
    src = EXAMPLE_RANKS + ".cpp"
    if force or _stale(EXAMPLE_RANKS, [src, LIBPGO, LIBGEN, os.path.join(INCLUDE, "pgo.h"), os.path.join(INCLUDE, "pgo_graphgen.h")]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", INCLUDE, "-o", EXAMPLE_RANKS, src, "-L", _HERE, "-l:libpgo.so", "-l:libpgo_graphgen.so", "-Wl,-rpath," + _HERE])
    return EXAMPLE_RANKS


def build_all(force=False):
    build_graphgen(force)
    build_libpgo(force)
    build_libpgo_sparse(force)
    build_host(force)
    build_examples(force)
    build_example_ranks(force)
