// pgo_sparse_blocks.hpp — the host side of libpgo_sparse.so's block interface (include/pgo_sparse.h) that needs no GPU: the undamped Schur complement S of a handle as
// 6 x 6 blocks from pgo_get_normal_blocks' arrays (sc_reduce_normal_blocks), the checks and the adjacency of a caller's pair list (sc_check_pairs, sc_pair_adjacency),
// where a 6 x 6 block lands in the permuted tile matrix (sc_block_entry: what the fill kernel computes per entry) and the right-hand sides of
// pgo_sparse_chol_inverse_blocks from its CSR rows (ScRows).  tests/native/sparse_companion_host.cpp runs all of it on the host.  For the selected inverse: where an
// entry of a 6 x 6 block of the inverse is stored (sc_sigma_entry) and the gather of a block on the host (sc_selected_block_host; tests/native/sparse_selinv_host.cpp).
// For the columns of the inverse in number (pgo_sparse_chol_inverse_columns): the chunks of column keyframes that fit the workspace (sc_column_chunks), the checked and
// laid-out request with its counts (ScColumns), the gather and the whole call on the host (sc_host_inverse_columns; tests/native/sparse_panel_host.cpp).
//
// S, per entry, is pgo_dense_math.hpp's arithmetic for a matrix-free handle (DcMfPlan, dc_mf_diag_entry, dc_mf_offdiag_entry): per keyframe H_ii minus c c^T / h over
// its switch sides in edge order; per pair of keyframes the sum in edge order (relative-pose before switchable) of J1^T J2 — transposed where the edge's c1 is the lower
// keyframe — minus c_hi c_lo^T / h for switchable edges.  Rows of the higher keyframe, columns of the lower.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "pgo_sparse_math.hpp"

namespace pgo {

struct ScReduced {
    std::vector<int32_t> pair_hi, pair_lo;      // unique, sorted by (hi, lo), hi > lo, both keyframes free
    std::vector<double> diag, blocks;           // [N][36] (zero for a keyframe that is not free), [pairs][36]
};
inline ScReduced sc_reduce_normal_blocks(int64_t N, const uint8_t* node_free, const double* diag, const double* offdiag, const double* sw_c, const double* sw_h, int64_t n_rel, const int32_t* rc1,
                                         const int32_t* rc2, int64_t n_sw, const int32_t* sc1, const int32_t* sc2) {
    const DcMfPlan M(N, node_free, n_rel, rc1, rc2, n_sw, sc1, sc2);
    ScReduced R;
    R.pair_hi = M.seg_hi; R.pair_lo = M.seg_lo;
    R.diag.assign((size_t)N * 36, 0.0);
    R.blocks.assign((size_t)M.segments() * 36, 0.0);
    for (int64_t i = 0; i < N; ++i) {
        if (!node_free[i]) continue;
        for (int a = 0; a < 6; ++a)
            for (int c = 0; c < 6; ++c)
                R.diag[(size_t)i * 36 + a * 6 + c] = dc_mf_diag_entry(diag + (size_t)i * 36, M.side.data(), M.side_ptr[(size_t)i], M.side_ptr[(size_t)i + 1], a, c, sw_c, sw_h);
    }
    for (int64_t s = 0; s < M.segments(); ++s)
        for (int a = 0; a < 6; ++a)
            for (int c = 0; c < 6; ++c)
                R.blocks[(size_t)s * 36 + a * 6 + c] = dc_mf_offdiag_entry(M.ent.data(), M.seg_ptr[(size_t)s], M.seg_ptr[(size_t)s + 1], a, c, offdiag, offdiag + (size_t)n_rel * 36, sw_c, sw_h);
    return R;
}

// a pair list as pgo_sparse_chol_create takes it: two distinct keyframes of the system each, no pair twice (in either order).  Returns nullptr, or what is wrong.
inline const char* sc_check_pairs(int64_t N, const uint8_t* in_system, int64_t n_pairs, const int32_t* hi, const int32_t* lo) {
    std::vector<std::pair<int32_t, int32_t>> seen;
    seen.reserve((size_t)n_pairs);
    for (int64_t k = 0; k < n_pairs; ++k) {
        const int32_t a = hi[k], b = lo[k];
        if (a < 0 || b < 0 || a >= N || b >= N) return "a pair names a keyframe out of range";
        if (a == b) return "a pair joins a keyframe with itself";
        if (!in_system[a] || !in_system[b]) return "a pair names a keyframe outside the system";
        seen.emplace_back(std::max(a, b), std::min(a, b));
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return "a pair of keyframes is listed twice";
    return nullptr;
}
// the neighbours of every keyframe, for sc_plan_graph
inline void sc_pair_adjacency(int64_t N, int64_t n_pairs, const int32_t* hi, const int32_t* lo, std::vector<int64_t>& adj_ptr, std::vector<int32_t>& adj) {
    adj_ptr.assign((size_t)N + 1, 0);
    for (int64_t k = 0; k < n_pairs; ++k) { ++adj_ptr[(size_t)hi[k] + 1]; ++adj_ptr[(size_t)lo[k] + 1]; }
    for (int64_t i = 0; i < N; ++i) adj_ptr[(size_t)i + 1] += adj_ptr[(size_t)i];
    adj.assign((size_t)adj_ptr[(size_t)N], 0);
    std::vector<int64_t> fill(adj_ptr.begin(), adj_ptr.end() - 1);
    for (int64_t k = 0; k < n_pairs; ++k) { adj[(size_t)fill[(size_t)hi[k]]++] = lo[k]; adj[(size_t)fill[(size_t)lo[k]]++] = hi[k]; }
}

// Entry (a, c) of the 6 x 6 block with its rows at keyframe position pr and its columns at position pc (pr != pc, or the diagonal block pr == pc): the row and column of
// the permuted matrix's LOWER triangle it belongs to — the block is read transposed where its rows come first.  false: the entry lies above the diagonal of a diagonal block.
PGO_DC_HD bool sc_block_entry(int32_t pr, int32_t pc, int a, int c, int* row, int* col) {
    const int r = pr * 6 + a, q = pc * 6 + c;
    if (pr == pc && c > a) return false;
    *row = r > q ? r : q; *col = r > q ? q : r;
    return true;
}

// the tiles of a block system on the host, as the fill kernel writes them: zeroed storage, the blocks under the permutation, ones on the diagonal of the rows outside the system and of the padding
inline void sc_fill_blocks_host(const ScPlan& P, int64_t N, const uint8_t* in_system, const int32_t* pos, const double* diag, int64_t n_pairs, const int32_t* hi, const int32_t* lo, const double* blocks, double* T) {
    std::fill(T, T + (size_t)P.tiles() * SC_TILE, 0.0);
    auto put = [&](int row, int col, double v) { T[(size_t)P.find(row / DC_NB, col / DC_NB) * SC_TILE + (size_t)(row % DC_NB) * DC_NB + col % DC_NB] = v; };
    int row, col;
    for (int64_t i = 0; i < N; ++i)
        for (int a = 0; a < 6; ++a)
            for (int c = 0; c < 6; ++c) {
                if (!sc_block_entry(pos[i], pos[i], a, c, &row, &col)) continue;
                if (in_system[i]) put(row, col, diag[(size_t)i * 36 + a * 6 + c]);
                else if (a == c) put(row, col, 1.0);
            }
    for (int i = (int)(N * 6); i < P.nt * DC_NB; ++i) put(i, i, 1.0);
    for (int64_t k = 0; k < n_pairs; ++k)
        for (int a = 0; a < 6; ++a)
            for (int c = 0; c < 6; ++c) { sc_block_entry(pos[hi[k]], pos[lo[k]], a, c, &row, &col); put(row, col, blocks[(size_t)k * 36 + a * 6 + c]); }
}

// Entry (i, j) of the 6 x 6 block of the inverse with its rows at keyframe position pr and its columns at position pc: the row and column of the permuted matrix's
// LOWER triangle that hold it (the inverse is symmetric; the selected inverse stores the lower tiles, and in a diagonal tile this is the lower half).  (pc, pr, j, i)
// gives the same place: (b, a) is the exact transpose of (a, b), a diagonal block is exactly symmetric.
PGO_DC_HD void sc_sigma_entry(int32_t pr, int32_t pc, int i, int j, int* row, int* col) {
    const int r = pr * 6 + i, q = pc * 6 + j;
    *row = r > q ? r : q; *col = r > q ? q : r;
}
// One block of the selected inverse Z (ScSelHost's tiles) on the host, as the gather kernel reads it: rows of keyframe a, columns of keyframe b, the caller's keyframe
// order.  A keyframe outside the system: a zero block (true).  A block may straddle up to four tiles — those of its four corners; false and zeros when one of them is
// not in the pattern.
inline bool sc_selected_block_host(const ScPlan& P, const double* Z, const uint8_t* in_system, const int32_t* pos, int32_t a, int32_t b, double* out36) {
    std::fill(out36, out36 + 36, 0.0);
    if (!in_system[a] || !in_system[b]) return true;
    int row, col;
    for (int i = 0; i < 6; i += 5)
        for (int j = 0; j < 6; j += 5) { sc_sigma_entry(pos[a], pos[b], i, j, &row, &col); if (P.find(row / DC_NB, col / DC_NB) < 0) return false; }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            sc_sigma_entry(pos[a], pos[b], i, j, &row, &col);
            out36[i * 6 + j] = Z[(size_t)P.find(row / DC_NB, col / DC_NB) * SC_TILE + (size_t)(row % DC_NB) * DC_NB + col % DC_NB];
        }
    return true;
}

// ---- pgo_sparse_chol_inverse_columns: blocks of the inverse between ANY keyframes, by the panel sweeps (sc_panel_steps) on the unit rows of the column keyframes.
// W of one chunk must fit the workspace limit; a panel of W is 64 rows of nc doubles, the least a limit may be.
inline int64_t sc_panel_bytes(int nc) { return (int64_t)DC_NB * nc * (int64_t)sizeof(double); }
// runs [begin, end) of the n_cols column keyframes (six rows each) whose W — whole panels — fits workspace_bytes; boundaries on whole keyframes.  Empty: the limit is
// below one panel.
inline std::vector<std::pair<int64_t, int64_t>> sc_column_chunks(int64_t n_cols, int nc, int64_t workspace_bytes) {
    std::vector<std::pair<int64_t, int64_t>> runs;
    const int64_t per = workspace_bytes / sc_panel_bytes(nc) * DC_NB / 6;      // >= 10 keyframes per panel
    if (per < 1) return runs;
    for (int64_t s = 0; s < n_cols; s += per) runs.emplace_back(s, std::min(n_cols, s + per));
    return runs;
}
struct ScColumnChunk {
    int m_pad = 0;                    // rows of W: a multiple of 64
    std::vector<int32_t> rhs_col;     // [m_pad]: the column of the row's one, ascending; -1: a padding row
    std::vector<int32_t> first;       // [m_pad / 64]: the tile of the panel's first one
    std::vector<int32_t> row0;        // [n_cols]: the first of the six rows of column keyframe col_node[c] in this chunk's W; -1: it has none here
};
// A request checked and laid out.  The column keyframes that a block with two keyframes of the system asks for get six unit rows each, in ascending POSITION (a keyframe
// may straddle two panels), dealt out in chunks; a block with a keyframe outside the system is zero and asks for nothing.  launches: per chunk the right-hand sides, the
// steps of the two sweeps and the gather; products: ScPlan::panel_products; workspace: bytes of the largest chunk's W.
struct ScColumns {
    const char* error = nullptr;
    std::vector<ScColumnChunk> chunks;
    int k_stop = 0;
    int64_t launches = 0, products = 0, workspace = 0;
    ScColumns(const ScPlan& P, int64_t N, const uint8_t* in_system, const int32_t* pos, int64_t n_cols, const int32_t* col_node, int64_t n_blocks, const int32_t* row_node,
              const int32_t* col_index, int64_t workspace_bytes) {
        const int nc = P.nt * DC_NB;
        std::vector<uint8_t> seen((size_t)N, 0), used((size_t)n_cols, 0);
        for (int64_t c = 0; c < n_cols; ++c) {
            if (col_node[c] < 0 || col_node[c] >= N) { error = "a column keyframe is out of range"; return; }
            if (seen[(size_t)col_node[c]]) { error = "a column keyframe is listed twice"; return; }
            seen[(size_t)col_node[c]] = 1;
        }
        for (int64_t k = 0; k < n_blocks; ++k) {
            if (row_node[k] < 0 || row_node[k] >= N) { error = "a row keyframe is out of range"; return; }
            if (col_index[k] < 0 || col_index[k] >= n_cols) { error = "a column index is out of range"; return; }
        }
        if (workspace_bytes < sc_panel_bytes(nc)) { error = "the workspace limit is below one panel of right-hand sides"; return; }
        k_stop = P.nt;
        for (int64_t k = 0; k < n_blocks; ++k)
            if (in_system[row_node[k]] && in_system[col_node[col_index[k]]]) { k_stop = std::min(k_stop, pos[row_node[k]] * 6 / DC_NB); used[(size_t)col_index[k]] = 1; }
        std::vector<int32_t> live;
        for (int64_t c = 0; c < n_cols; ++c) if (used[(size_t)c]) live.push_back((int32_t)c);
        std::sort(live.begin(), live.end(), [&](int32_t a, int32_t b) { return pos[col_node[a]] < pos[col_node[b]]; });
        for (const auto& run : sc_column_chunks((int64_t)live.size(), nc, workspace_bytes)) {
            ScColumnChunk C;
            C.m_pad = (int)(((run.second - run.first) * 6 + DC_NB - 1) / DC_NB * DC_NB);
            C.rhs_col.assign((size_t)C.m_pad, -1);
            C.row0.assign((size_t)n_cols, -1);
            int32_t r = 0;
            for (int64_t q = run.first; q < run.second; ++q) {
                const int32_t c = live[(size_t)q];
                C.row0[(size_t)c] = r;
                for (int a = 0; a < 6; ++a) C.rhs_col[(size_t)r++] = pos[col_node[c]] * 6 + a;
            }
            for (int p = 0; p < C.m_pad / DC_NB; ++p) C.first.push_back(C.rhs_col[(size_t)p * DC_NB] / DC_NB);
            launches += 2 + P.panel_launches(C.first.data(), (int)C.first.size(), k_stop);
            products += P.panel_products(C.first.data(), (int)C.first.size(), k_stop);
            workspace = std::max(workspace, (int64_t)C.m_pad * nc * (int64_t)sizeof(double));
            chunks.push_back(std::move(C));
        }
    }
};
// entry (i, j) of block k out of one chunk's W, as the gather kernel reads it: rows of keyframe row_node[k], the six right-hand sides of column col_index[k].  out is
// zeroed before the first chunk: a block with a keyframe outside the system stays zero.
inline void sc_columns_gather_host(const ScColumnChunk& C, const double* W, int nc, const uint8_t* in_system, const int32_t* pos, int64_t n_blocks, const int32_t* row_node,
                                   const int32_t* col_index, double* out) {
    for (int64_t k = 0; k < n_blocks; ++k) {
        const int32_t r0 = C.row0[(size_t)col_index[k]];
        if (r0 < 0 || !in_system[row_node[k]]) continue;
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) out[k * 36 + i * 6 + j] = W[(size_t)(r0 + j) * nc + (size_t)pos[row_node[k]] * 6 + i];
    }
}
#if !defined(__HIP_DEVICE_COMPILE__)
// the whole call on the host, on the factored tiles T: what pgo_sparse_chol_inverse_columns does chunk by chunk
inline void sc_host_inverse_columns(const ScPlan& P, const double* T, const ScColumns& Q, const uint8_t* in_system, const int32_t* pos, int64_t n_blocks, const int32_t* row_node,
                                    const int32_t* col_index, double* out) {
    const int nc = P.nt * DC_NB;
    std::fill(out, out + n_blocks * 36, 0.0);
    for (const ScColumnChunk& C : Q.chunks) {
        std::vector<double> W((size_t)C.m_pad * nc, 0.0);
        for (int r = 0; r < C.m_pad; ++r) if (C.rhs_col[(size_t)r] >= 0) W[(size_t)r * nc + C.rhs_col[(size_t)r]] = 1.0;
        ScPanelHost H{P, T, W.data(), nc, C.first.data()};
        sc_panel_steps(P, C.first, Q.k_stop, H);
        sc_columns_gather_host(C, W.data(), nc, in_system, pos, n_blocks, row_node, col_index, out);
    }
}
#endif

// The right-hand sides of pgo_sparse_chol_inverse_blocks: groups of 1 or 6 sparse rows in CSR over the 6 N coordinates of the caller's keyframe order.  Per non-zero its
// place in W [rows][nc] under the permutation; first_tile: the first tile that holds a non-zero of any row (nt: there is none).
struct ScRows {
    int64_t rows = 0;
    std::vector<int32_t> first_row, dim;        // per group
    std::vector<int64_t> at; std::vector<double> val;
    int first_tile = 0;
    const char* error = nullptr;
    ScRows(int64_t N, const uint8_t* in_system, const int32_t* pos, int nc, int64_t n_groups, const int64_t* group_ptr, const int64_t* row_ptr, const int32_t* col, const double* v) {
        first_tile = nc / DC_NB;
        if (n_groups < 1 || group_ptr[0] != 0) { error = "the groups do not start at row 0"; return; }
        for (int64_t g = 0; g < n_groups; ++g) {
            const int64_t d = group_ptr[g + 1] - group_ptr[g];
            if (d != 1 && d != 6) { error = "a group has neither 1 nor 6 rows"; return; }
            first_row.push_back((int32_t)group_ptr[g]); dim.push_back((int32_t)d);
        }
        rows = group_ptr[n_groups];
        if (row_ptr[0] != 0) { error = "the rows do not start at entry 0"; return; }
        for (int64_t r = 0; r < rows; ++r) {
            if (row_ptr[r + 1] < row_ptr[r]) { error = "the row pointers descend"; return; }
            for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
                const int32_t c = col[e];
                if (c < 0 || c >= N * 6) { error = "a column is out of range"; return; }
                if (e > row_ptr[r] && c <= col[e - 1]) { error = "the columns of a row do not ascend"; return; }
                if (!in_system[c / 6]) { error = "a row has an entry on a keyframe outside the system"; return; }
                const int p = pos[c / 6] * 6 + c % 6;
                at.push_back(r * (int64_t)nc + p); val.push_back(v[e]);
                first_tile = std::min(first_tile, p / DC_NB);
            }
        }
    }
};

}  // namespace pgo
