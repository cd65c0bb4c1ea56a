// pgo_graph.hip — from the handle's host edge lists to the device graph: the edge classes in K1's layout, the keyframes' incident lists and block-CSR pattern, the matrix-free
// operator's workgroup tiles, the work buffers and the device descriptors bound to them (build_graph), and the entry of edges into the host lists (add_edges).
//
// build_graph is a driver over stages.  The stages that work on the host alone take host vectors and constants and return host structs — no handle, no HIP call — so that
// what an upload reads, and until when, stands in the driver.  What it replaces in the reference: the `ceres::Problem` bookkeeping calls of
// PoseGraphSLAM::reinit_ceres_problem_onnewloopedge_optimize6DOF (src/PoseGraphSLAM.cpp:1340-1367,1550-1556,1629-1633,1803-1849).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "pgo_handle.hpp"

namespace {

// Matrix4d (column-major 16) -> Meas fields
void meas_from_matrix(const double* T, double w, double* out8) {
    double R[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r * 3 + c] = T[c * 4 + r];
    double q[4];
    eigen_matrix_to_quat(R, q);   // CeresResidues.h:24 / :150
    out8[0] = q[0]; out8[1] = q[1]; out8[2] = q[2]; out8[3] = q[3];
    out8[4] = T[12]; out8[5] = T[13]; out8[6] = T[14]; out8[7] = w;
}

// the caller's keyframe index -> this handle's (several ranks: the rank-local numbering, -1 for a keyframe this rank does not touch; one GPU: the same index)
struct LocalIndex {
    const int32_t* g2l;
    int32_t operator()(int32_t g) const { return g2l ? g2l[g] : g; }
};

// ---- stage: validate against the array sizes the caller solves with; sw_used[i] = switch i belongs to an edge of this handle.  Returns the error's text, or nullptr.
const char* validate(const HostClass& rel, const HostClass& swe, const std::vector<PriorDev>& priors, int64_t N, int64_t S, std::vector<uint8_t>& sw_used) {
    for (const HostClass* H : {&rel, &swe})
        for (int64_t e = 0; e < H->size(); ++e)
            if (H->c1[e] < 0 || H->c1[e] >= N || H->c2[e] < 0 || H->c2[e] >= N) return "edge endpoint out of range for n_nodes";
    sw_used.assign((size_t)S, 0);
    for (int64_t e = 0; e < swe.size(); ++e) {
        const int32_t si = swe.sw[e];
        if (si < 0 || si >= S) return "switch index out of range for n_switch";
        if (sw_used[si]) return "switch index used by more than one edge";
        sw_used[si] = 1;
    }
    for (const PriorDev& pr : priors) if (pr.node < 0 || pr.node >= N) return "regulariser node out of range";
    return nullptr;
}

// ---- stage: free flags.  A keyframe is part of the program when a residual block touches it: on one GPU that is a non-empty incident list (known before the lists are built:
// the hierarchy's worker starts on these flags); in a rank-local subgraph every keyframe is touched by construction (by this rank or, for the stand-in keyframe of an idle rank,
// possibly by none: `touched_any`, over the caller's keyframes, with `l2g` — both unused on one GPU).  Constant keyframes are not free.
std::vector<uint8_t> free_flags(const HostClass& rel, const HostClass& swe, const std::vector<PriorDev>& priors, const std::vector<int32_t>& constant_nodes, LocalIndex L,
                                int64_t N, int64_t N_global, const std::vector<int32_t>& l2g, const std::vector<uint8_t>& touched_any) {
    std::vector<uint8_t> touched_here((size_t)N, 0), node_free((size_t)N, 0);
    for (const HostClass* H : {&rel, &swe}) for (int64_t e = 0; e < H->size(); ++e) { touched_here[L(H->c1[e])] = 1; touched_here[L(H->c2[e])] = 1; }
    for (const PriorDev& pr : priors) touched_here[L(pr.node)] = 1;
    for (int64_t n = 0; n < N; ++n) node_free[n] = (touched_here[n] || (L.g2l && touched_any[l2g[n]])) ? 1 : 0;
    for (int32_t c : constant_nodes) if (c >= 0 && c < N_global && L(c) >= 0) node_free[L(c)] = 0;
    return node_free;
}

// ---- stage: one edge class in K1's layout — SoA planes padded to whole tiles of TILE edges, the pose window of every tile
struct PackedClass {
    std::vector<int32_t> c1, c2, sw;
    std::vector<double> meas;
    std::vector<double> loss;      // [Epad] encoded robust loss in the edges' packed order, or empty: no edge of the class carries one
    std::vector<int4> win;
    int64_t E = 0, Epad = 0;
    int tiles() const { return (int)win.size(); }
};
PackedClass pack_class(const HostClass& H, bool is_sw, LocalIndex L) {
    PackedClass P;
    const int64_t E = P.E = H.size();
    const int64_t Epad = P.Epad = (E + TILE - 1) / TILE * TILE;
    const int tiles = (int)(Epad / TILE);
    P.c1.resize(Epad); P.c2.resize(Epad); P.sw.resize(is_sw ? Epad : 0); P.meas.resize((size_t)8 * Epad); P.win.resize(tiles);
    if (std::any_of(H.loss.begin(), H.loss.end(), [](double a) { return a != 0.0; })) P.loss.assign((size_t)Epad, 0.0);
    for (int64_t e = 0; e < Epad; ++e) {
        const int64_t s = e < E ? e : E - 1;   // padding lanes replicate the last edge (computed, never stored or counted)
        P.c1[e] = L(H.c1[s]); P.c2[e] = L(H.c2[s]);
        if (is_sw) P.sw[e] = H.sw[s];
        if (!P.loss.empty() && s < (int64_t)H.loss.size()) P.loss[e] = H.loss[s];      // the plane goes with the edge, wherever the packing puts it
        for (int k = 0; k < 8; ++k) P.meas[(size_t)k * Epad + e] = H.meas[(size_t)s * 8 + k];
    }
    for (int t = 0; t < tiles; ++t) {
        int lo1 = INT32_MAX, hi1 = -1, lo2 = INT32_MAX, hi2 = -1;
        for (int l = 0; l < TILE; ++l) {
            const int64_t e = (int64_t)t * TILE + l;
            lo1 = std::min(lo1, P.c1[e]); hi1 = std::max(hi1, P.c1[e]); lo2 = std::min(lo2, P.c2[e]); hi2 = std::max(hi2, P.c2[e]);
        }
        const int n1 = hi1 - lo1 + 1, n2 = hi2 - lo2 + 1;
        P.win[t] = make_int4(lo1, n1 <= WIN_MAX ? n1 : 0, lo2, n2 <= WIN_MAX ? n2 : 0);
    }
    return P;
}

// ---- stage: keyframe -> incident list (edges in slot order, then regularisers) and the block-CSR pattern (row n: block (n, n), then one block per incident edge).  An incident
// entry is (slot << 1) | side; slots: relative-pose edges, from rel_Epad the switchable edges, from rel_Epad + sw_Epad the regularisers.
struct IncidentLists {
    std::vector<int64_t> rowptr, inc, bsr_rowptr;
    std::vector<int32_t> bsr_col;
    std::vector<PriorDev> priors;      // the regularisers on this handle's keyframe indices
    int64_t nnzb() const { return bsr_rowptr.back(); }
};
IncidentLists incident_lists(const HostClass& rel, const HostClass& swe, const std::vector<PriorDev>& priors, LocalIndex L, int64_t N, int64_t rel_Epad, int64_t sw_Epad) {
    IncidentLists I;
    const int64_t Er = rel.size(), Es = swe.size(), Eg = (int64_t)priors.size();
    I.priors = priors;
    for (PriorDev& x : I.priors) x.node = L(x.node);
    std::vector<int64_t>& rowptr = I.rowptr; std::vector<int64_t>& bsr_rowptr = I.bsr_rowptr;
    rowptr.assign(N + 1, 0); bsr_rowptr.assign(N + 1, 0);
    for (int64_t e = 0; e < Er; ++e) { rowptr[L(rel.c1[e]) + 1]++; rowptr[L(rel.c2[e]) + 1]++; }
    for (int64_t e = 0; e < Es; ++e) { rowptr[L(swe.c1[e]) + 1]++; rowptr[L(swe.c2[e]) + 1]++; }
    for (int64_t n = 0; n < N; ++n) bsr_rowptr[n + 1] = bsr_rowptr[n] + 1 + rowptr[n + 1];
    for (int64_t k = 0; k < Eg; ++k) rowptr[I.priors[k].node + 1]++;
    for (int64_t n = 0; n < N; ++n) rowptr[n + 1] += rowptr[n];
    I.inc.resize((size_t)rowptr[N]); I.bsr_col.resize((size_t)bsr_rowptr[N]);
    std::vector<int64_t> fill(rowptr.begin(), rowptr.end() - 1), bfill(N);
    for (int64_t n = 0; n < N; ++n) { I.bsr_col[bsr_rowptr[n]] = (int32_t)n; bfill[n] = bsr_rowptr[n] + 1; }
    auto add_edge = [&](int64_t slot, int32_t a, int32_t b) {
        I.inc[fill[a]++] = (slot << 1) | 0; I.bsr_col[bfill[a]++] = b;
        I.inc[fill[b]++] = (slot << 1) | 1; I.bsr_col[bfill[b]++] = a;
    };
    for (int64_t e = 0; e < Er; ++e) add_edge(e, L(rel.c1[e]), L(rel.c2[e]));
    for (int64_t e = 0; e < Es; ++e) add_edge(rel_Epad + e, L(swe.c1[e]), L(swe.c2[e]));
    for (int64_t k = 0; k < Eg; ++k) I.inc[fill[I.priors[k].node]++] = ((rel_Epad + sw_Epad + k) << 1);
    return I;
}

// ---- stage: may the matrix-free operator serve this graph?  A keyframe with more edge sides than a workgroup tile holds (a hub revisited hundreds of times), or with several
// regularisers, is served by the assembled block-CSR operator instead.
bool matrix_free_eligible(const IncidentLists& I, int64_t N, int64_t slot_pr0) {
    for (int64_t n = 0; n < N; ++n) {
        int64_t deg = 0, npri = 0;
        for (int64_t k = I.rowptr[n]; k < I.rowptr[n + 1]; ++k) { if ((I.inc[k] >> 1) >= slot_pr0) ++npri; else ++deg; }
        if (deg > MF_BLOCK || npri > 1) return false;
    }
    return true;
}

// ---- stage: the matrix-free operator's tiles — edge sides in keyframe-major order, packed into workgroup tiles of whole keyframes
struct MfTiles {
    std::vector<int32_t> tile_node0;            // [tiles + 1] first keyframe of every tile
    std::vector<int64_t> tile_inc0;             // [tiles + 1] first lane of every tile
    std::vector<int32_t> tile_sw0;              // [tiles] first switchable lane inside the tile | pair lanes << 16
    std::vector<uint32_t> einc, eslot;          // per lane: edge << 1 | side (bit 31: switchable); slot of the side | slot of a pair's side 1 << 9 | keyframe inside the tile << 18
    std::vector<int32_t> eoth;                  // per lane: the other keyframe
    std::vector<ushort4> node_rng;              // per keyframe: slot ranges of its relative-pose sides (x, y) and of its switchable sides (z, w)
    std::vector<int32_t> node_prior;            // per keyframe: its regulariser, or -1
    int64_t pair_lanes = 0, rel_side_lanes = 0, sw_lanes = 0;      // lanes by kind (pgo_time_kernel's bytes)
    int tiles() const { return (int)tile_node0.size() - 1; }
};
// Returns the error's text, or nullptr.
const char* pack_mf_tiles(const IncidentLists& I, const HostClass& rel, const HostClass& swe, LocalIndex L, int64_t N, int64_t rel_Epad, int64_t sw_Epad, MfTiles& M) {
    const std::vector<int64_t>& rowptr = I.rowptr; const std::vector<int64_t>& inc = I.inc;
    const int64_t Er = rel.size(), Es = swe.size();
    // per keyframe: its relative-pose sides and its switchable sides (both in incident-list order), regulariser index
    std::vector<int32_t> deg_rel(N, 0), deg_sw(N, 0);
    M.node_prior.assign(N, -1);
    const int64_t slot_pr = rel_Epad + sw_Epad;
    for (int64_t n = 0; n < N; ++n) {
        for (int64_t k = rowptr[n]; k < rowptr[n + 1]; ++k) {
            const int64_t slot = inc[k] >> 1;
            if (slot >= slot_pr) {
                if (M.node_prior[n] >= 0) return "matrix-free operator: more than one regulariser on a keyframe";
                M.node_prior[n] = (int32_t)(slot - slot_pr);
            } else if (slot >= rel_Epad) ++deg_sw[n]; else ++deg_rel[n];
        }
        if (deg_rel[n] + deg_sw[n] > MF_BLOCK) return "matrix-free operator: a keyframe with more incident edges than a matrix-free tile holds (use PGO_LINEAR_PCG_BLOCK_JACOBI)";
    }
    if ((int64_t)std::max(Er, Es) >= (1ll << 30)) return "matrix-free operator: more than 2^30 edges in one class";
    // pack whole keyframes into workgroup tiles: <= MF_SLOTS edge sides, <= MF_BLOCK lanes (a relative-pose edge with both keyframes in
    // the tile takes ONE lane for its two sides), <= MF_MAX_NODES keyframes
    auto rel_other_of = [&](int64_t k) -> int32_t {      // incident entry k of a relative-pose side: the other keyframe, or -1
        const int64_t slot = inc[k] >> 1; const int side = (int)(inc[k] & 1);
        if (slot >= rel_Epad) return -1;
        const int32_t a = L(rel.c1[slot]), b = L(rel.c2[slot]);
        return a == b ? -1 : (side == 0 ? b : a);
    };
    std::vector<int32_t>& tile_node0 = M.tile_node0;
    tile_node0.assign(1, 0);
    { int64_t sides = 0, pairs = 0; int cur_nodes = 0; int32_t start = 0;
      for (int64_t n = 0; n < N; ++n) {
          const int64_t d = deg_rel[n] + deg_sw[n];
          auto pairs_with = [&](int32_t lo) { int64_t c = 0; for (int64_t k = rowptr[n]; k < rowptr[n + 1]; ++k) { const int32_t o = rel_other_of(k); if (o >= lo && o < (int32_t)n) ++c; } return c; };
          int64_t np = pairs_with(start);
          if (sides + d > MF_SLOTS || sides + d - (pairs + np) > MF_BLOCK || cur_nodes >= MF_MAX_NODES) {
              tile_node0.push_back((int32_t)n); sides = 0; pairs = 0; cur_nodes = 0; start = (int32_t)n; np = 0;
          }
          sides += d; pairs += np; ++cur_nodes;
      }
      tile_node0.push_back((int32_t)N); }
    const int tiles = M.tiles();
    std::vector<int64_t>& tile_inc0 = M.tile_inc0; std::vector<int32_t>& tile_sw0 = M.tile_sw0;
    std::vector<uint32_t>& einc = M.einc; std::vector<uint32_t>& eslot = M.eslot; std::vector<int32_t>& eoth = M.eoth; std::vector<ushort4>& node_rng = M.node_rng;
    tile_inc0.assign(tiles + 1, 0);
    tile_sw0.assign(std::max(tiles, 1), 0);
    node_rng.resize(std::max<int64_t>(N, 1));
    einc.reserve((size_t)(Er + 2 * Es) + 64); eoth.reserve(einc.capacity()); eslot.reserve(einc.capacity());
    std::vector<uint16_t> side_slot((size_t)(rowptr[N]), 0);       // slot of incident entry k inside its tile
    std::vector<uint16_t> rel_slot1((size_t)std::max<int64_t>(Er, 1), 0);   // per relative-pose edge: slot of its side 1 (own = c2)
    for (int t = 0; t < tiles; ++t) {
        const int32_t n0 = tile_node0[t], n1 = tile_node0[t + 1];
        tile_inc0[t] = (int64_t)einc.size();
        // slots: the keyframes' relative-pose sides, then their switchable sides, each in incident-list order
        int slot_n = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int32_t n = n0; n < n1; ++n) {
                const unsigned short begin = (unsigned short)slot_n;
                for (int64_t k = rowptr[n]; k < rowptr[n + 1]; ++k) {
                    const int64_t slot = inc[k] >> 1;
                    if (slot >= slot_pr || (int)(slot >= rel_Epad) != pass) continue;
                    side_slot[k] = (uint16_t)slot_n;
                    if (pass == 0 && (inc[k] & 1)) rel_slot1[slot] = (uint16_t)slot_n;
                    ++slot_n;
                }
                if (pass == 0) { node_rng[n].x = begin; node_rng[n].y = (unsigned short)slot_n; } else { node_rng[n].z = begin; node_rng[n].w = (unsigned short)slot_n; }
            }
        // lanes: pairs, then the other relative-pose sides, then the switchable sides
        int n_pairs = 0;
        for (int group = 0; group < 3; ++group) {
            if (group == 2) tile_sw0[t] = (int32_t)(((int64_t)einc.size() - tile_inc0[t]) | ((int64_t)n_pairs << 16));
            for (int32_t n = n0; n < n1; ++n)
                for (int64_t k = rowptr[n]; k < rowptr[n + 1]; ++k) {
                    const int64_t slot = inc[k] >> 1; const int side = (int)(inc[k] & 1);
                    if (slot >= slot_pr) continue;
                    const bool is_sw = slot >= rel_Epad;
                    if (is_sw != (group == 2)) continue;
                    const int64_t e = is_sw ? slot - rel_Epad : slot;
                    const int32_t a = L(is_sw ? swe.c1[e] : rel.c1[e]), b = L(is_sw ? swe.c2[e] : rel.c2[e]);
                    const int32_t other = side == 0 ? b : a;
                    const bool paired = !is_sw && a != b && other >= n0 && other < n1;
                    if (group == 0) {
                        if (!paired || side != 0) continue;          // the pair's lane stands at side 0 (own = c1)
                        einc.push_back((uint32_t)(e << 1));
                        eoth.push_back(b);
                        eslot.push_back((uint32_t)side_slot[k] | ((uint32_t)rel_slot1[e] << 9) | ((uint32_t)(n - n0) << 18));
                        ++n_pairs;
                    } else {
                        if (group == 1 && paired) continue;
                        einc.push_back((is_sw ? 0x80000000u : 0u) | (uint32_t)(e << 1) | (uint32_t)side);
                        eoth.push_back(other);
                        eslot.push_back((uint32_t)side_slot[k] | (511u << 9) | ((uint32_t)(n - n0) << 18));
                    }
                }
        }
    }
    tile_inc0[tiles] = (int64_t)einc.size();
    for (int t = 0; t < tiles; ++t) { M.pair_lanes += (uint32_t)tile_sw0[t] >> 16; M.sw_lanes += (tile_inc0[t + 1] - tile_inc0[t]) - (tile_sw0[t] & 0xffff); }
    M.rel_side_lanes = (int64_t)einc.size() - M.pair_lanes - M.sw_lanes;
    return nullptr;
}

// ---- uploads.  Each waits for its copies: the host struct may go when it returns.
int upload_class(pgo_problem* p, const PackedClass& P, DBuf<int32_t>& dc1, DBuf<int32_t>& dc2, DBuf<int32_t>* dsw, DBuf<double>& dmeas, DBuf<int4>& dwin, EdgeClassDev& out) {
    const bool robust = !P.loss.empty();      // (a class with a robust edge)
    DBuf<double>& dloss = dsw ? p->d_sloss : p->d_rloss;
    DBuf<double>& dlossc = dsw ? p->d_slossc : p->d_rlossc;
    if (P.Epad > 0) {
        HIPCHK(p, dc1.upload(P.c1, p->st)); HIPCHK(p, dc2.upload(P.c2, p->st)); HIPCHK(p, dmeas.upload(P.meas, p->st)); HIPCHK(p, dwin.upload(P.win, p->st));
        if (dsw) HIPCHK(p, dsw->upload(P.sw, p->st));
        if (robust) { HIPCHK(p, dloss.upload(P.loss, p->st)); HIPCHK(p, dlossc.ensure((size_t)P.Epad)); }
        HIPCHK(p, hipStreamSynchronize(p->st));
    }
    out.c1 = dc1.p; out.c2 = dc2.p; out.meas = dmeas.p; out.swidx = dsw ? dsw->p : nullptr; out.win = dwin.p;
    out.E = P.E; out.Epad = P.Epad; out.tiles = P.tiles(); out.J = nullptr;
    out.loss = robust ? dloss.p : nullptr; out.lossc = robust ? dlossc.p : nullptr;
    return PGO_OK;
}

int upload_incident_lists(pgo_problem* p, const IncidentLists& I) {
    HIPCHK(p, p->d_inc_rowptr.upload(I.rowptr, p->st)); HIPCHK(p, p->d_bsr_rowptr.upload(I.bsr_rowptr, p->st)); HIPCHK(p, p->d_inc.upload(I.inc, p->st));
    HIPCHK(p, p->d_bsr_col.upload(I.bsr_col, p->st)); HIPCHK(p, p->d_node_free.upload(p->h_node_free, p->st)); HIPCHK(p, p->d_prior.upload(I.priors, p->st));
    HIPCHK(p, hipStreamSynchronize(p->st));
    return PGO_OK;
}

// ... and binds the matrix-free operator's descriptor (p->F) and records its lane counts
int upload_mf_tiles(pgo_problem* p, const MfTiles& M) {
    const int64_t ninc_e = (int64_t)M.einc.size();
    const int64_t ninc_pad = (ninc_e + 63) / 64 * 64 + 64;
    HIPCHK(p, p->d_einc.upload(M.einc, p->st)); HIPCHK(p, p->d_einc_slot.upload(M.eslot, p->st)); HIPCHK(p, p->d_einc_other.upload(M.eoth, p->st));
    HIPCHK(p, p->d_node_rng.upload(M.node_rng, p->st)); HIPCHK(p, p->d_tile_inc0.upload(M.tile_inc0, p->st)); HIPCHK(p, p->d_tile_node0.upload(M.tile_node0, p->st));
    HIPCHK(p, p->d_tile_sw0.upload(M.tile_sw0, p->st)); HIPCHK(p, p->d_node_prior.upload(M.node_prior, p->st));
    HIPCHK(p, p->d_rec.ensure((size_t)MF_PLANES * ninc_pad)); HIPCHK(p, p->d_lam.ensure(std::max<int64_t>(p->N * 6, 1)));
    HIPCHK(p, hipStreamSynchronize(p->st));
    p->mf_pair_lanes = M.pair_lanes; p->mf_sw_lanes = M.sw_lanes; p->mf_rel_side_lanes = M.rel_side_lanes;
    p->F = MfDev{p->d_einc.p, p->d_einc_other.p, p->d_einc_slot.p, p->d_tile_inc0.p, p->d_tile_sw0.p, p->d_tile_node0.p, p->d_node_rng.p, p->d_node_prior.p,
                 p->d_rec.p, p->d_lam.p, ninc_e, ninc_pad, M.tiles()};
    return PGO_OK;
}

// ---- stage: work buffers (allocation only) and the device descriptors bound to them
int allocate_work_buffers(pgo_problem* p) {
    const GraphDev& G = p->G;
    const int64_t N = p->N, S = p->S, Es = G.sw.E, Eg = (int64_t)p->priors.size(), slots = G.rel.Epad + G.sw.Epad;
    const bool mf = p->built_mf;
    HIPCHK(p, p->d_Jr.ensure(std::max<int64_t>((int64_t)G.rel.tiles * REL_DOUBLES * TILE, 1)));
    HIPCHK(p, p->d_Js.ensure(std::max<int64_t>((int64_t)G.sw.tiles * SW_DOUBLES * TILE, 1)));
    HIPCHK(p, p->d_Jp.ensure(std::max<int64_t>(Eg * PRIOR_DOUBLES, 1)));
    HIPCHK(p, p->d_Hd_g.ensure(std::max<int64_t>(N * 42, 1)));
    HIPCHK(p, p->d_Hoff.ensure(mf ? 1 : std::max<int64_t>(slots * 36, 1)));
    HIPCHK(p, p->d_c.ensure(std::max<int64_t>(Es * 12, 1))); HIPCHK(p, p->d_hss.ensure(std::max<int64_t>(Es, 1))); HIPCHK(p, p->d_gs.ensure(std::max<int64_t>(Es, 1)));
    HIPCHK(p, p->d_scale_p.ensure(std::max<int64_t>(N * 6, 1))); HIPCHK(p, p->d_diag_p.ensure(std::max<int64_t>(N * 6, 1)));
    HIPCHK(p, p->d_scale_s.ensure(std::max<int64_t>(Es, 1))); HIPCHK(p, p->d_diag_s.ensure(std::max<int64_t>(Es, 1))); HIPCHK(p, p->d_a_inv.ensure(std::max<int64_t>(Es, 1)));
    if (G.sw.lossc) HIPCHK(p, p->d_a_inv_mf.ensure(std::max<int64_t>(Es, 1)));
    HIPCHK(p, p->d_val.ensure(mf ? 1 : std::max<int64_t>(p->nnzb * 36, 1))); HIPCHK(p, p->d_Lf.ensure(std::max<int64_t>(N * 24 + 64 * 24, 1))); HIPCHK(p, p->d_Dtot_b.ensure(std::max<int64_t>(N * 42, 1)));
    HIPCHK(p, p->d_cgvec.ensure(std::max<int64_t>(N * 42, 1)));
    p->n_part = std::max<int64_t>(MAX_PARTIALS, (G.rel.tiles + G.sw.tiles + 3) / 4 + 1);
    HIPCHK(p, p->d_part.ensure(p->n_part * 6));
    HIPCHK(p, p->d_cgpart.ensure(PQ_SLOTS + 2 * RZ_STRIDE + 16));   // partial sums + 16 PCG scalars (C.scal)
    HIPCHK(p, p->d_flags.ensure(8)); HIPCHK(p, p->d_scal.ensure(S_N));
    for (int k = 0; k < 2; ++k) { HIPCHK(p, p->d_pose[k].ensure(std::max<int64_t>(N * 8, 1))); HIPCHK(p, p->d_swv[k].ensure(std::max<int64_t>(S, 1))); }
    HIPCHK(p, p->d_delta_s.ensure(std::max<int64_t>(Es, 1))); HIPCHK(p, p->d_io.ensure(std::max<int64_t>(N * 7, 1)));
    return PGO_OK;
}
void bind_descriptors(pgo_problem* p) {
    GraphDev& G = p->G;
    const int64_t N = p->N;
    G.rel.J = p->d_Jr.p; G.sw.J = p->d_Js.p;
    G.prior = p->d_prior.p; G.n_prior = (int32_t)p->priors.size(); G.Jp = p->d_Jp.p;
    G.inc_rowptr = p->d_inc_rowptr.p; G.inc = p->d_inc.p; G.node_free = p->d_node_free.p;
    G.bsr_rowptr = p->d_bsr_rowptr.p; G.bsr_col = p->d_bsr_col.p; G.nnzb = p->nnzb;
    p->L = LinDev{p->d_Hd_g.p, p->d_Hd_g.p + (size_t)N * 36, p->d_Hoff.p, p->d_c.p, p->d_hss.p, p->d_gs.p};
    p->Sc = ScaleDev{p->d_scale_p.p, p->d_scale_s.p, p->d_diag_p.p, p->d_diag_s.p, p->d_a_inv.p};
    p->ScMf = p->Sc;
    if (G.sw.lossc) p->ScMf.a_inv = p->d_a_inv_mf.p;
    CgDev& C = p->C;
    C.val = p->d_val.p; C.Lf = p->d_Lf.p; C.Dtot = p->d_Dtot_b.p; C.b = p->d_Dtot_b.p + (size_t)N * 36;
    double* v = p->d_cgvec.p; const size_t n6 = (size_t)N * 6;
    C.x = v; C.r = v + n6; C.r2 = v + 2 * n6; C.z = v + 3 * n6; C.p = v + 4 * n6; C.p2 = v + 5 * n6; C.q = v + 6 * n6;
    C.part_pq = p->d_cgpart.p; C.part_rz = p->d_cgpart.p + PQ_SLOTS; C.scal = p->d_cgpart.p + PQ_SLOTS + 2 * RZ_STRIDE; C.extra_rz = 0;
    C.flags = p->d_flags.p;
}

}  // namespace

namespace pgo {

int add_edges(pgo_problem* p, HostClass& H, int64_t n, const int32_t* c1, const int32_t* c2, const double* T, const double* w, const int32_t* sw, double loss_enc) {
    if (n < 0 || (n > 0 && (!c1 || !c2 || !T))) { p->err = "null edge array"; return PGO_ERR_INVALID_ARG; }
    for (int64_t k = 0; k < n; ++k) if (c1[k] < 0 || c2[k] < 0 || c1[k] == c2[k] || (sw && sw[k] < 0)) { p->err = "negative index or self edge"; return PGO_ERR_INVALID_ARG; }
    mg_drop_pending(p);      // (the worker reads the edge lists)
    const size_t base = H.c1.size();
    H.c1.insert(H.c1.end(), c1, c1 + n);
    H.c2.insert(H.c2.end(), c2, c2 + n);
    if (sw) H.sw.insert(H.sw.end(), sw, sw + n);
    H.meas.resize((base + n) * 8);
    for (int64_t k = 0; k < n; ++k) meas_from_matrix(T + 16 * k, w ? w[k] : 1.0, &H.meas[(base + k) * 8]);
    if (loss_enc != 0.0 && n > 0) { H.loss.resize(base, 0.0); H.loss.resize(base + n, loss_enc); }      // (trivial edges never touch the plane: see HostClass)
    p->graph_dirty = true;
    return PGO_OK;
}

// The device graph of the handle's edge lists for `N` keyframes and `S` switches (sw_now: the switch values the solve starts from: the hierarchy's coupling strengths).
// What the order of the stages must keep:
//   * Worker thread.  One GPU: the HOST half of the multigrid hierarchy (pgo_mg_host.hpp: ~0.1 s for C3, single-threaded sorts and matchings) needs the edge lists and the free
//     flags only, so mg_start_fresh starts it on a worker thread once the free flags are final and before the edge classes are uploaded; it runs beside the stages that follow and
//     is installed where build_multigrid used to compute it (nothing depends on timing: the result is the same hierarchy).  From mg_start_fresh until build_multigrid returns
//     nothing writes p->rel, p->swe, p->priors, p->h_node_free, p->g2l or p->l2g: the stages in between take them by const reference and return structs of their own.
//   * Guard.  An early return after mg_start_fresh waits for the worker and drops its result.
//   * Collectives.  Every rank issues the same collectives in the same order: the sum all-reduce and the max all-reduce of number_rank_local, then whatever build_multigrid
//     issues (several ranks: its host half holds collectives, so it runs there, synchronously).
int build_graph(pgo_problem* p, int64_t N, int64_t S, const double* sw_now) {
    mg_drop_pending(p);      // (a worker reads the host arrays rebuilt below)
    double t_phase = now_s();
    auto phase = [&](const char* what) { if (p->opt.verbosity > 1) { const double t = now_s(); std::fprintf(stderr, "[pgo] build_graph: %-34s %7.2f ms\n", what, (t - t_phase) * 1e3); t_phase = t; } };
    auto fail = [&](const char* text) { p->err = text; return PGO_ERR_INVALID_ARG; };
    int rc;
    if (const char* bad = validate(p->rel, p->swe, p->priors, N, S, p->h_sw_used)) return fail(bad);
    p->S = S; p->N_global = N;
    GraphDev& G = p->G;
    G = GraphDev{};
    if ((rc = number_rank_local(p, p->N_global, &N)) != PGO_OK) return rc;      // several ranks: N = this rank's keyframes from here on
    p->N = N;
    phase("validation, rank-local numbering");
    const LocalIndex L{p->local_ids ? p->g2l.data() : nullptr};
    G.N = N; G.S = S;
    p->h_node_free = free_flags(p->rel, p->swe, p->priors, p->constant_nodes, L, N, p->N_global, p->l2g, p->h_touched_any);

    struct Guard { pgo_problem* p; bool committed = false; ~Guard() { if (!committed) mg_drop_pending(p); } } mg_guard{p};
    mg_start_fresh(p, sw_now);
    if ((rc = upload_class(p, pack_class(p->rel, false, L), p->d_rc1, p->d_rc2, nullptr, p->d_rmeas, p->d_rwin, G.rel)) != PGO_OK) return rc;
    if ((rc = upload_class(p, pack_class(p->swe, true, L), p->d_sc1, p->d_sc2, &p->d_sidx, p->d_smeas, p->d_swin, G.sw)) != PGO_OK) return rc;
    phase("edge classes packed + uploaded");

    const IncidentLists I = incident_lists(p->rel, p->swe, p->priors, L, N, G.rel.Epad, G.sw.Epad);
    p->nnzb = I.nnzb();
    if ((rc = upload_incident_lists(p, I)) != PGO_OK) return rc;
    phase("incident lists + block-CSR structure");

    p->built_mf = p->opt.linear_solver == PGO_LINEAR_PCG_MATRIX_FREE && matrix_free_eligible(I, N, G.rel.Epad + G.sw.Epad);
    p->F = MfDev{};
    if (p->built_mf) {
        MfTiles M;
        if (const char* bad = pack_mf_tiles(I, p->rel, p->swe, L, N, G.rel.Epad, G.sw.Epad, M)) return fail(bad);
        if ((rc = upload_mf_tiles(p, M)) != PGO_OK) return rc;
    }
    phase("matrix-free tiles");

    if ((rc = allocate_work_buffers(p)) != PGO_OK) return rc;
    bind_descriptors(p);
    if (dense_mode(p)) { if ((rc = dense_allocate(p)) != PGO_OK) return rc; }
    else dense_release(p);
    phase("work buffers");

    // ---- the preconditioner of this graph: the aggregation multigrid for large graphs — a hierarchy of graph-following rigid aggregates (pgo_mg_host.hpp), built by
    // build_multigrid(), which a solve may call again with the current switch values (regroup) — or the two-level method
    if ((rc = build_multigrid(p, sw_now)) != PGO_OK) return rc;      // (one GPU: only announced, the hierarchy is on the worker)
    phase("multigrid hierarchy");
    if (p->mg.built && p->built_mf) { HIPCHK(p, p->d_Hoff.ensure((size_t)(p->G.rel.Epad + p->G.sw.Epad) * 36)); p->L.Hoff = p->d_Hoff.p; }      // the multigrid's level-1 product reads J1^T J2 per edge
    p->hoff_epoch = 0;
    if (dense_mode(p)) {
        // no aggregates, and no memory of them: the two-level method's history across solves (kept / dropped, back-off) counts CONSECUTIVE solves that used it, and a graph built
        // for the exact solver ends every such run — a handle that goes back to a PCG afterwards starts where a fresh handle starts (solves before and after are bitwise equal)
        p->coarse.hist = CoarseState::History{};
    }
    if (!p->mg.built && !dense_mode(p) && (rc = build_two_level_aggregates(p)) != PGO_OK) return rc;      // (a graph that got the multigrid never uses the two-level method: its dense operator would be built and uploaded for nothing)
    phase("two-level aggregates");
    mg_guard.committed = true;
    p->graph_dirty = false; p->priors_dirty = false;
    ++p->pcg.build_epoch;   // invalidates the captured PCG graph (kernel arguments hold device pointers / sizes)
    return PGO_OK;
}

}  // namespace pgo
