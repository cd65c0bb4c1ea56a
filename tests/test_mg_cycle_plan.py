"""CPU: the multigrid cycle's plan (csrc/pgo_mg_cycle.hpp: mg_cycle_plan), instantiated on the host by tests/native/mg_cycle_host.cpp, against step lists written out
here.  The lists are the specification — the sequence of launches and exchange points the cycle makes on a hierarchy of each shape, in the order the launcher made them
before the plan existed.  launch_mg_apply walks the plan, choose_split picks the riders' hosts from it: what is pinned here is what both see.

A hierarchy is given as (tiles_own, rT_tiles, smoothed, explicit transfer) per sparse level; level n_levels is the dense one.  In every case: 70 level-1 aggregates to restrict
to (three workgroups of 32 rows) unless stated, 5 workgroups of the dense solve, 7 workgroups of the PCG's vector kernels.

For every case also: the rider-eligible launches and their workgroups equal what the enumeration choose_split used to read (rider_hosts_reference below, kept here as the
reference only), and the kernel steps number at most 2 n_levels + 1 + 2 n_sm — the bound chunk_length (pgo_pcg.hip) cuts captured chunks by.

The shim built with a main of its own runs the same cases once under -fsanitize=address,undefined, as a stand-alone program."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "solve_keyframe_pose_graph_amd", "csrc")
SRC = os.path.join(HERE, "native", "mg_cycle_host.cpp")
GXX = ["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I", CSRC]
N1, N_AGG, CG_GRID, MAX_PARTIALS = 70, 5, 7, 1024


def _stale(target):
    deps = [SRC, os.path.join(CSRC, "pgo_mg_cycle.hpp"), os.path.join(CSRC, "pgo_internal.hpp")]
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in deps)


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "native", "libmg_cycle_host.so")
    if _stale(so):
        subprocess.check_call(GXX + ["-O2", "-fPIC", "-shared", "-o", so, SRC])
    return C.CDLL(so)


def X(point, level):
    return ("exchange", level, point, 0, False)


def L(kind, level, grid, rider=False):
    return (kind, level, -1, grid, rider)


R = True      # the launch can carry riders

PLAIN2 = [(40, 0, 0, 0)]
PLAIN3 = [(40, 0, 0, 0), (6, 0, 0, 0)]
IMPL3 = [(40, 0, 1, 0), (6, 0, 0, 0)]
EXPL3 = [(40, 9, 1, 1), (6, 0, 0, 0)]
WIDE2 = [(2100, 0, 0, 0)]                        # more level-1 tiles than r.z partial slots
IDLE_MIDDLE3 = [(40, 0, 0, 0), (0, 0, 0, 0)]     # several ranks: this rank owns no tile of level 2
IDLE_EXPL3 = [(40, 0, 0, 0), (0, 0, 1, 1)]       # ... of an explicit-transfer level 2, and no coarse row of its restriction either
RESTRICT_ONLY_EXPL3 = [(40, 0, 0, 0), (0, 4, 1, 1)]      # ... no tile, but four tiles of coarse rows to restrict to

RESTRICT0 = [L("restrict0", 1, 3)]

# name -> (levels, options, the steps AFTER the restriction, the restriction's own step when the update has not restricted already)
CASES = {
    "one level": ([], {}, [X(0, 1), L("dense_solve", 1, 5), X(2, 1), L("prolong0", 1, 7)], RESTRICT0),
    "two levels": (PLAIN2, {},
                   [X(0, 1), L("down", 1, 40, R), X(0, 2), L("dense_solve", 2, 5), X(1, 1), L("up", 1, 40, R), X(2, 1), L("prolong0", 1, 7)], RESTRICT0),
    "two levels, fused": (PLAIN2, dict(extra_rz=40),
                          [X(0, 1), L("down", 1, 40, R), X(0, 2), L("dense_solve", 2, 5), X(1, 1), L("up_fused", 1, 40), X(2, 1)], RESTRICT0),
    "two levels, fused, more tiles than slots": (WIDE2, dict(extra_rz=MAX_PARTIALS),
                                                 [X(0, 1), L("down", 1, 2100, R), X(0, 2), L("dense_solve", 2, 5), X(1, 1), L("up_fused", 1, MAX_PARTIALS), X(2, 1)], RESTRICT0),
    "three levels": (PLAIN3, {},
                     [X(0, 1), L("down", 1, 40, R), X(0, 2), L("down", 2, 6, R), X(0, 3), L("dense_solve", 3, 5),
                      X(1, 2), L("up", 2, 6, R), X(1, 1), L("up", 1, 40, R), X(2, 1), L("prolong0", 1, 7)], RESTRICT0),
    "three levels, fused": (PLAIN3, dict(extra_rz=40),
                            [X(0, 1), L("down", 1, 40, R), X(0, 2), L("down", 2, 6, R), X(0, 3), L("dense_solve", 3, 5),
                             X(1, 2), L("up", 2, 6, R), X(1, 1), L("up_fused", 1, 40), X(2, 1)], RESTRICT0),
    "three levels, implicit smoothed level 1": (IMPL3, {},
                                                [X(0, 1), L("pre_smooth", 1, 40), L("down", 1, 40, R), X(0, 2), L("down", 2, 6, R), X(0, 3), L("dense_solve", 3, 5),
                                                 X(1, 2), L("up", 2, 6, R), X(1, 1), L("post_smooth", 1, 40), L("up", 1, 40, R), X(2, 1), L("prolong0", 1, 7)], RESTRICT0),
    "three levels, implicit smoothed level 1, fused": (IMPL3, dict(extra_rz=40),
                                                       [X(0, 1), L("pre_smooth", 1, 40), L("down", 1, 40, R), X(0, 2), L("down", 2, 6, R), X(0, 3), L("dense_solve", 3, 5),
                                                        X(1, 2), L("up", 2, 6, R), X(1, 1), L("post_smooth", 1, 40), L("up_fused", 1, 40), X(2, 1)], RESTRICT0),
    # sdown: the level's 40 tiles and the 9 tiles of coarse rows its restriction runs on, one launch; its up launch (which reads the next level's x itself) has the 40
    "three levels, explicit level 1": (EXPL3, {},
                                       [X(0, 1), L("sdown", 1, 49, R), X(0, 2), L("down", 2, 6, R), X(0, 3), L("dense_solve", 3, 5),
                                        X(1, 2), L("up", 2, 6, R), X(1, 1), L("up", 1, 40, R), X(2, 1), L("prolong0", 1, 7)], RESTRICT0),
    "three levels, explicit level 1, fused": (EXPL3, dict(extra_rz=40),
                                              [X(0, 1), L("sdown", 1, 49, R), X(0, 2), L("down", 2, 6, R), X(0, 3), L("dense_solve", 3, 5),
                                               X(1, 2), L("up", 2, 6, R), X(1, 1), L("up_fused", 1, 40), X(2, 1)], RESTRICT0),
    # the keyframe level's transfer view (11 tiles of coarse rows): restriction and prolongation by kernels of their own; the update never restricts for it
    "fine view, one level": ([], dict(fine=11), [X(0, 1), L("dense_solve", 1, 5), X(2, 1), L("prolong_fine", 1, 7)], [L("restrict_fine", 1, 11)]),
    "fine view, two levels": (PLAIN2, dict(fine=11),
                              [X(0, 1), L("down", 1, 40, R), X(0, 2), L("dense_solve", 2, 5), X(1, 1), L("up", 1, 40, R), X(2, 1), L("prolong_fine", 1, 7)], [L("restrict_fine", 1, 11)]),
    # several ranks (the update never restricts there): the exchange points stay, the launches go
    "three levels, no tile of level 2": (IDLE_MIDDLE3, dict(ranks=True),
                                         [X(0, 1), L("down", 1, 40, R), X(0, 2), X(0, 3), L("dense_solve", 3, 5), X(1, 2), X(1, 1), L("up", 1, 40, R), X(2, 1), L("prolong0", 1, 7)], RESTRICT0),
    "three levels, no aggregate to restrict to": (IDLE_MIDDLE3, dict(ranks=True, n1=0),
                                                  [X(0, 1), L("down", 1, 40, R), X(0, 2), X(0, 3), L("dense_solve", 3, 5), X(1, 2), X(1, 1), L("up", 1, 40, R), X(2, 1), L("prolong0", 1, 7)], []),
    "three levels, explicit level 2 without tiles or coarse rows": (IDLE_EXPL3, dict(ranks=True),
                                                                    [X(0, 1), L("down", 1, 40, R), X(0, 2), X(0, 3), L("dense_solve", 3, 5), X(1, 2), X(1, 1), L("up", 1, 40, R), X(2, 1), L("prolong0", 1, 7)], RESTRICT0),
    "three levels, explicit level 2 with coarse rows only": (RESTRICT_ONLY_EXPL3, dict(ranks=True),
                                                             [X(0, 1), L("down", 1, 40, R), X(0, 2), L("sdown", 2, 4, R), X(0, 3), L("dense_solve", 3, 5),
                                                              X(1, 2), X(1, 1), L("up", 1, 40, R), X(2, 1), L("prolong0", 1, 7)], RESTRICT0),
}


def runs():
    """(id, levels, shim arguments, expected steps): every case with the restriction as a step of the cycle and — where the solver has that combination: one GPU, no fine view —
    with the restriction inside the vector update"""
    out = []
    for name, (levels, opt, steps, restriction) in CASES.items():
        args = dict(n1=opt.get("n1", N1), extra_rz=opt.get("extra_rz", 0), fine=opt.get("fine", -1))
        out.append((name, levels, dict(args, restricted=0), restriction + steps))
        if "fine" not in opt and not opt.get("ranks"):
            out.append((name + ", restricted", levels, dict(args, restricted=1), steps))
    return out


RUNS = runs()


def rider_hosts_reference(levels, extra_rz):
    """the enumeration of rider-eligible launches the split update's rule read before the plan existed (mg_rider_hosts), line for line: their own workgroups in launch order"""
    fused = extra_rz > 0
    tiles = []
    for tiles_own, rT_tiles, smoothed, explicit in levels:
        if smoothed and explicit:
            if tiles_own + rT_tiles > 0:
                tiles.append(tiles_own + rT_tiles)
        elif tiles_own > 0:
            tiles.append(tiles_own)
    for l in range(len(levels), 0, -1):
        tiles_own = levels[l - 1][0]
        if tiles_own == 0 or (l == 1 and fused):
            continue
        tiles.append(tiles_own)
    return tiles


def plan(shim, levels, n1, extra_rz, fine, restricted):
    cap = shim.mgc_capacity()
    lv = (C.c_int * max(1, 4 * len(levels)))(*[v for level in levels for v in level])
    rows, names, hosts = (C.c_int * (4 * cap))(), (C.c_char_p * cap)(), C.c_int(-1)
    n = shim.mgc_plan(len(levels) + 1, lv, n1, N_AGG, extra_rz, CG_GRID, restricted, fine, rows, names, C.byref(hosts))
    assert 0 < n <= cap
    return [(names[i].decode(), rows[4 * i], rows[4 * i + 1], rows[4 * i + 2], bool(rows[4 * i + 3])) for i in range(n)], hosts.value


@pytest.mark.parametrize("name,levels,args,expected", RUNS, ids=[r[0] for r in RUNS])
def test_the_plan_is_the_written_out_step_list(shim, name, levels, args, expected):
    steps, hosts = plan(shim, levels, **args)
    assert steps == expected
    eligible = [s[3] for s in steps if s[4]]
    assert hosts == len(eligible) and eligible == rider_hosts_reference(levels, args["extra_rz"])
    n_levels = len(levels) + 1
    n_sm = sum(1 for _, _, smoothed, explicit in levels if smoothed and not explicit)
    assert sum(1 for s in steps if s[0] != "exchange") <= 2 * n_levels + 1 + 2 * n_sm


def test_the_deepest_hierarchy_fits_the_plan(shim):
    """MG_MAX_LEVELS levels, every sparse one with an implicit smoothed prolongator, unfused: six steps per sparse level and five around them — the plan's capacity"""
    n_levels = shim.mgc_max_levels()
    steps, hosts = plan(shim, [(3, 0, 1, 0)] * (n_levels - 1), n1=N1, extra_rz=0, fine=-1, restricted=0)
    assert len(steps) == 6 * (n_levels - 1) + 5 == shim.mgc_capacity()
    assert hosts == 2 * (n_levels - 1)


def test_the_same_cases_in_a_sanitized_stand_alone_program(shim, tmp_path):
    exe = str(tmp_path / "mg_cycle_host_san")
    subprocess.check_call(GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMGC_MAIN", "-o", exe, SRC])
    n_max = shim.mgc_max_levels()      # (asked of the unsanitized shim; the program under the sanitizers is a process of its own)
    deepest = ("deepest", [(3, 0, 1, 0)] * (n_max - 1), dict(n1=N1, extra_rz=0, fine=-1, restricted=0), None)
    lines = []
    for _, levels, a, _ in RUNS + [deepest]:
        lines.append(" ".join(str(v) for v in [len(levels) + 1, a["n1"], N_AGG, a["extra_rz"], CG_GRID, a["restricted"], a["fine"]] + [v for level in levels for v in level]))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stderr == ""
    got = out.stdout.splitlines()
    assert len(got) == len(RUNS) + 1
    for line, (_, levels, a, expected) in zip(got, RUNS):
        head, _, rest = line.partition(":")
        steps = [tuple(f.split(",")) for f in rest.split()]
        steps = [(k, int(lv), int(pt), int(g), r == "1") for k, lv, pt, g, r in steps]
        assert steps == expected, head
        assert int(head.split()[3]) == len(rider_hosts_reference(levels, a["extra_rz"]))
