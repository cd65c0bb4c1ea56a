"""Builds libpgo of a git revision into build/variants/libpgo_<name>.so, for bit-for-bit comparisons of a new build against an older one on the same box:
PGO_LIBPGO_OVERRIDE=build/variants/libpgo_<name>.so python -m tests.solve_digest C3 ...
  python scripts/dev/build_rev.py <revision> <name>
The revision's own _build.py, csrc and include are taken with `git archive` and built by that revision's compile_libpgo (objects under build/rev_obj/<name>): the variant is
byte for byte what a checkout of that revision builds, whatever translation units it has."""
import importlib.util, io, os, shutil, subprocess, sys, tarfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
rev, name = sys.argv[1], sys.argv[2]
src = os.path.join(ROOT, "build", "rev_src", name)
shutil.rmtree(src, ignore_errors=True)
os.makedirs(src)
tar = subprocess.check_output(["git", "archive", rev, "solve_keyframe_pose_graph_amd/_build.py", "solve_keyframe_pose_graph_amd/csrc", "include"], cwd=ROOT)
tarfile.open(fileobj=io.BytesIO(tar)).extractall(src)
spec = importlib.util.spec_from_file_location("rev_build_" + name, os.path.join(src, "solve_keyframe_pose_graph_amd", "_build.py"))
rev_build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rev_build)
out = os.path.join(ROOT, "build", "variants", "libpgo_%s.so" % name)
os.makedirs(os.path.dirname(out), exist_ok=True)
rev_build.compile_libpgo(out, obj_dir=os.path.join(ROOT, "build", "rev_obj", name))
print(out)
