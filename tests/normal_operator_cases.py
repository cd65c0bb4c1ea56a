"""The graphs tests/test_normal_operator_ref.py (CPU) and tests/test_gpu_normal_operator.py (GPU) share: small chains (util.small_graph(N, 0, f=1)) with extra edges that
drive the matrix-free operator's tile packing (pack_mf_tiles, csrc/pgo_graph.hip) to its edges — a tile closed by the lane limit, a keyframe of exactly 256 edge sides, a
tile without lanes, a last tile of one keyframe, parallel and reversed edges, a relative-pose and a switchable edge on one pair, pairs straddling a tile boundary, constant
keyframes at a boundary — and the two graphs that must fall back to the assembled operator (degree 257, two regularisers on one keyframe).

Extra edges are measured between the TRUE poses with small seeded noise (non-zero residuals), weights spread over 0.1 .. 3; the state is initial_state(perturb = 0.02).
Every case names the tile condition it is built for (normal_operator_ref.tile_condition): the CPU test shows it with the Python restatement of the closing rule, the GPU
test asserts it again on the tables the device holds."""
import functools
from dataclasses import dataclass, field

import numpy as np

from tests import util

RADII = (1e4, 1e-2)      # the second: a damping-dominated system
PERTURB, STATE_SEED = 0.02, 6
BIG = (44000, 4400, 1, 11)      # small_graph arguments of the graph with more than MF_MAX_GRID tiles


@dataclass
class Graph:
    name: str
    n_poses: int
    init_q: np.ndarray
    init_t: np.ndarray
    rel_c1: np.ndarray
    rel_c2: np.ndarray
    rel_T: np.ndarray
    rel_w: np.ndarray
    sw_c1: np.ndarray
    sw_c2: np.ndarray
    sw_T: np.ndarray
    sw_w: np.ndarray
    reg_node: np.ndarray
    reg_T: np.ndarray
    reg_w: np.ndarray
    constant: tuple = ()
    condition: str = None          # normal_operator_ref.tile_condition
    matrix_free: bool = True       # linear_solver = 1 serves it with the matrix-free operator (False: the assembled fall-back)
    notes: dict = field(default_factory=dict)

    @property
    def n_sw(self):
        return len(self.sw_c1)


def _pose_matrices(g):
    return util.poses_to_matrices(g.truth_q, g.truth_t).reshape(-1, 4, 4).transpose(0, 2, 1)      # column-major rows -> [n, 4, 4]


def _measure(M, a, b, rng):
    """c1_T_c2 = M_a^-1 M_b of the true poses, with a small rotation and translation error; [n, 16] column-major"""
    out = np.zeros((len(a), 16))
    for k, (i, j) in enumerate(zip(a, b)):
        T = np.linalg.inv(M[i]) @ M[j]
        w = rng.normal(size=3) * 0.004
        th = np.linalg.norm(w)
        K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
        E = np.eye(4); E[:3, :3] = R; E[:3, 3] = rng.normal(size=3) * 0.02
        out[k] = (T @ E).flatten(order="F")
    return out


def _build(name, N, seed, rel=(), sw=(), regs=(), drop=None, **kw):
    """chain of N keyframes + extra relative-pose pairs `rel`, switchable pairs `sw`, extra regularised keyframes `regs`; drop(c1, c2) -> mask of chain edges to leave out"""
    g = util.small_graph(N, 0, f=1, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    M = _pose_matrices(g)
    keep = np.ones(g.n_odom, bool) if drop is None else ~drop(g.odom_c1, g.odom_c2)
    I32 = lambda x: np.asarray(x, dtype=np.int32).reshape(-1)
    rel = np.asarray(rel, np.int64).reshape(-1, 2); sw = np.asarray(sw, np.int64).reshape(-1, 2)
    rel_c1 = np.concatenate([g.odom_c1[keep], I32(rel[:, 0])]); rel_c2 = np.concatenate([g.odom_c2[keep], I32(rel[:, 1])])
    rel_T = np.concatenate([g.odom_T[keep], _measure(M, rel[:, 0], rel[:, 1], rng)])
    rel_w = np.concatenate([g.odom_w[keep], rng.uniform(0.1, 3.0, size=len(rel))])
    sw_T = _measure(M, sw[:, 0], sw[:, 1], rng)
    sw_w = rng.uniform(0.1, 3.0, size=len(sw))
    regs = I32(regs)
    reg_node = np.concatenate([g.reg_node, regs])
    reg_T = np.concatenate([g.reg_T, util.poses_to_matrices(g.truth_q[regs], g.truth_t[regs]) if len(regs) else np.zeros((0, 16))])
    reg_w = np.concatenate([g.reg_w, rng.uniform(0.5, 3.0, size=len(regs))])
    return Graph(name, N, g.init_q, g.init_t, rel_c1, rel_c2, rel_T, rel_w, I32(sw[:, 0]), I32(sw[:, 1]), sw_T, sw_w, reg_node, reg_T, reg_w, **kw)


def _lane_loops():
    return [(k, 150 + (7 * (6 * k + j)) % 150) for k in range(120) for j in range(6)]


def _hub(h, n_extra, seed, N=300):
    """n_extra distinct partners of keyframe h, none of them its chain neighbours"""
    rng = np.random.default_rng(seed)
    cand = np.array([n for n in range(N) if abs(n - h) > 1])
    return np.sort(rng.choice(cand, size=n_extra, replace=False))


def _alternate(h, partners):
    return [(h, o) if k % 2 == 0 else (o, h) for k, o in enumerate(partners)]


def _boundary(N, constant=()):
    rel = [(41, 42), (42, 41), (41, 42)]      # the chain's own edge on this pair is (42, 41): four parallel edges in both orientations across the first tile boundary
    sw = [(41, 42), (42, 41)]                 # ... and a switchable edge each way on the same pair
    return _build("boundary N=%d%s" % (N, " constant" if constant else ""), N, 3, rel=rel, sw=sw, constant=tuple(constant), condition="single")


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "lanes-sw":
        return _build(name, 300, 1, sw=_lane_loops(), condition="lanes250")
    if name == "lanes-rel":
        return _build(name, 300, 1, rel=[(a, b) if k % 2 == 0 else (b, a) for k, (a, b) in enumerate(_lane_loops())], condition="lanes250")
    if name == "hub256":
        return _build(name, 300, 2, rel=_alternate(137, _hub(137, 254, 5)), regs=[137], condition="lanes256")
    if name == "hub256-parallel":
        p = _hub(137, 127, 6)
        return _build(name, 300, 2, rel=[e for o in p for e in ((137, o), (o, 137))], condition="lanes256")
    if name == "hub200-mixed":
        h = 150
        near = [n for n in range(h - 50, h + 52) if abs(n - h) > 1][:99]      # 99 relative-pose partners around the hub: most of them share its tile
        far = [n for n in list(range(0, 60)) + list(range(240, 300))][:99]    # 99 switchable partners far away
        return _build(name, 300, 4, rel=_alternate(h, near), sw=_alternate(h, far), condition="pairs2")
    if name == "gap":
        in_gap = lambda c: (c >= 100) & (c <= 189)
        return _build(name, 300, 7, rel=[(99, 190)], drop=lambda c1, c2: in_gap(c1) | in_gap(c2), condition="empty")
    if name == "boundary43":
        return _boundary(43)
    if name == "boundary85":
        return _boundary(85)
    if name == "boundary43-constant":
        return _boundary(43, (41, 42))
    if name == "boundary85-constant":
        return _boundary(85, (41, 42))
    if name == "tiny2":
        return _build(name, 2, 8)
    if name == "tiny3-constant":
        return _build(name, 3, 8, constant=(1,))
    if name == "two-priors":
        return _build(name, 60, 9, regs=[17, 17], matrix_free=False)
    if name == "hub257":
        return _build(name, 300, 2, rel=_alternate(137, _hub(137, 255, 5)), regs=[137], matrix_free=False)
    raise KeyError(name)


SMALL = ("lanes-sw", "lanes-rel", "hub256", "hub256-parallel", "hub200-mixed", "gap", "boundary43", "boundary85", "boundary43-constant", "boundary85-constant",
         "tiny2", "tiny3-constant", "two-priors", "hub257")


@functools.lru_cache(maxsize=None)
def big_graph():
    """small_graph(44000, 4400, f=1): more than MF_MAX_GRID = 1024 tiles, not a multiple of it — some workgroups of the matvec make two trips, the others one"""
    g = util.small_graph(BIG[0], BIG[1], f=BIG[2], seed=BIG[3])
    return Graph("big44000", g.n_poses, g.init_q, g.init_t, g.odom_c1, g.odom_c2, g.odom_T, g.odom_w, g.loop_c1, g.loop_c2, g.loop_T, g.loop_w, g.reg_node, g.reg_T, g.reg_w)


def state(G):
    rng = np.random.default_rng(STATE_SEED)
    q = G.init_q + rng.normal(size=G.init_q.shape) * PERTURB
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = G.init_t + rng.normal(size=G.init_t.shape) * PERTURB
    s = np.full(G.n_sw, 0.99) + rng.normal(size=G.n_sw) * PERTURB      # reference src/PoseGraphSLAM.cpp:353
    return q, t, s


def oracle_problem(G):
    from oracle import binding as ob
    O = ob.OracleProblem()
    O.add_relpose_edges(G.rel_c1, G.rel_c2, G.rel_T, G.rel_w)
    if G.n_sw:
        O.add_switchable_edges(G.sw_c1, G.sw_c2, G.sw_T, G.sw_w, np.arange(G.n_sw))
    O.set_node_regularizers(G.reg_node, G.reg_T, G.reg_w)
    return O


def pgo_problem(G, **opt):
    from solve_keyframe_pose_graph_amd import capi
    P = capi.Problem(**opt)
    P.add_relpose_edges(G.rel_c1, G.rel_c2, G.rel_T, G.rel_w)
    if G.n_sw:
        P.add_switchable_edges(G.sw_c1, G.sw_c2, G.sw_T, G.sw_w, np.arange(G.n_sw, dtype=np.int32))
    P.set_node_regularizers(G.reg_node, G.reg_T, G.reg_w)
    if G.constant:
        P.set_nodes_constant(list(G.constant))
    return P


@functools.lru_cache(maxsize=None)
def reference(name, radius):
    """the sparse reference of a case at one radius (computed once per process, never modified)"""
    from tests import normal_operator_ref as nr
    G = big_graph() if name == "big44000" else graph(name)
    q, t, s = state(G)
    return nr.reference(oracle_problem(G), G, q, t, s, radius)
