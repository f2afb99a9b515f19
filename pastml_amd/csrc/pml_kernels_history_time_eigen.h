// Exact expected dwell times, Markov jumps and lineage counts per time interval for the eigen-decomposed models (JTT,
// CUSTOM_RATES, HKY handed over as an eigen model), all columns of a call in one pass (pml_history_through_time_eigen):
// pml_kernels_history_eigen.h's sums with every branch cut at the boundaries of the time bins.
//
// The host plans the cut (pml_time_segments.h): a segment is the part [s1, s1 + w] of a branch n, as fractions of the branch,
// that lies in one bin; r is what is left below it.  In the notation of pml_kernels_history_eigen.h, with u measured from the
// parent, the integral Phi_cd restricted to the segment factorises exactly:
//     Phi_cd^seg = exp(d_c s1 t') Phi_cd(w t') exp(d_d r t')                        (every exponent <= 0)
// so per segment, with y = w t',
//     ls[c] = l_n[c] exp(d_c s1 t'),   Ey[c] = exp(d_c y),   rs[d] = r_n[d] exp(d_d r t')
//     X_seg[c][d] = ls[c] Phi_cd(y) rs[d]              (heig_Phi on y, Ey: the same switch at |z| = 0.5, the same 15 terms)
//     W_m = sum of X_seg over the segments of bin m
//     times[m][s]    = (1 / sf) sum_cd Ainv[c][s] W_m[c][d] A[s][d]
//     jumps[m][i][j] = Q_ij sum_cd Ainv[c][i] W_m[c][d] A[j][d]                     (i != j; the diagonal exactly 0)
// A branch with t' = 0 has l_n = 0 staged and adds nothing; a branch without extent is one segment s1 = 0, w = 1, r = 0, whose
// ls, Ey, rs are l_n, E_n, r_n in bits (exp(0) = 1).  A segment whose branch is alive at the boundary its bin begins with
// (flagged by the plan; the point segments of the pseudo-bin M for the last boundary) adds, with s = frac[0], u = frac[3],
//     lineages[m][j] += (sum_c Ainv[c][j] l_n[c] exp(d_c s t')) (sum_d A[j][d] r_n[d] exp(d_d u t'))      (sums to 1 over j)
// and q_p[j] where t' = 0 (the formula at P = I; l_n is 0 there by design).
//
// heig_basis_kernel stages E_n, r_n, l_n and t'_n per branch as it does for the whole tree.  hte_segment_kernel forms ls, Ey, rs
// once per segment (3 k exponentials, 3 ks doubles), for heig_basis_kernel's reason: no pair may cost a transcendental.
// hte_pair_kernel has heig_pair_kernel's tiles and epilogue (heig_tile, heig_tile_sums) and a walk of its own over the segments
// of a piece of the plan (pml_cut_time_pieces by PML_HEIG_PIECE: no piece straddles two bins), without the per-branch sums.  The
// partials are summed in piece order per bin (hte_reduce_kernel), and times / jumps come from W_m by the two small products of
// pml_kernels_history_eigen_shared.h per bin (hte_t1_kernel, hte_times_kernel, hte_jumps_kernel).
// hte_lineage_kernel takes the flagged segments of a boundary in tiles of 16 -- the two changes of basis Ainv^T (l o e^{d s t'})
// and A (r o e^{d u t'}) by heig_product, on the FP64 matrix cores from 16 states on -- and adds the tiles of a piece of 512
// in tile order; hte_lineage_sum_kernel adds the pieces of a boundary in piece order and clamps at 0.
//
// Bits.  No floating-point atomics.  The plan sorts the segments by (bin, caller's id); pieces and tiles are cut per bin, a fixed
// number of segments whatever k is; a wavefront's segments, the order of its additions and the order in which wavefronts,
// tiles and pieces are combined are fixed.  So a bin's sums see the same pieces in the same order whatever other bins the call
// has, and nothing depends on the grid, on the other columns, on the column's position or on which outputs are asked for (W_m
// is formed in full either way).  The posteriors this reads are the eigen sweeps': their bits follow the schedule.
#pragma once
#include "pml_kernels_history_eigen_shared.h"

#define PML_HTE_TILE 16   // flagged segments per tile of the lineage kernel (the vectors of one MFMA operand)

struct PmlHteArgs {
    PmlHeigArgs h;                  // the vectors of the marginal pass, the model, N, k, ks, W, col0; stage and tprime
    int M;                          // time bins
    int n_segments;                 // the segments of the bins 0 .. M - 1
    int n_pieces;
    const int* seg_node;            // [n_segments] caller's id
    const double* seg_frac;         // [n_segments][4]: s1, w, r, u
    const int* piece_off;           // [n_pieces + 1]
    const int* bin_piece_off;       // [M + 1]
    int n_lpieces;
    const int* lin_node;            // [flagged] caller's id: the flagged segments by (boundary, id), the pseudo-bin M included
    const double* lin_frac;         // [flagged][4]
    const int* lpiece_off;          // [n_lpieces + 1]
    const int* bin_lpiece_off;      // [M + 2]
    double* sstage;                 // [cols][n_segments][3][ks]: Ey, rs, ls (the order of h.stage)
    double* sy;                     // [cols][n_segments]: y = w t'
    double* partial;                // [cols][n_pieces][k][k]
    double* Wsum;                   // [cols][M][k][k]
    double* T1;                     // [cols][M][k][k]
    double* lpart;                  // [cols][n_lpieces][k]
    double* times_out;              // [cols][M][k]
    double* jumps_out;              // [cols][M][k][k], or null
    double* lineages_out;           // [cols][M + 1][k], or null
};

// ls, Ey, rs and y of every segment.  grid (ceil(n_segments k / 256), column): a thread owns one state of one segment
static __global__ void __launch_bounds__(256) hte_segment_kernel(PmlHteArgs T) {
    const PmlHeigArgs& A = T.h;
    const int k = A.k, ks = A.ks;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)T.n_segments * k) return;
    const size_t i = idx / k;
    const int c = (int)(idx % k);
    const int id = T.seg_node[i];
    const double t = A.tprime[(size_t)blockIdx.y * A.N + id];
    const double s1 = T.seg_frac[4 * i], w = T.seg_frac[4 * i + 1], rr = T.seg_frac[4 * i + 2];
    const double d = A.ev[(size_t)(A.col0 + blockIdx.y) * k + c];
    const double* st = A.stage + ((size_t)blockIdx.y * A.N + id) * 3 * ks;
    double* out = T.sstage + ((size_t)blockIdx.y * T.n_segments + i) * 3 * ks;
    const double y = w * t;
    out[c] = exp(d * y);
    out[ks + c] = st[ks + c] * exp(d * (rr * t));
    out[2 * ks + c] = st[2 * ks + c] * exp(d * (s1 * t));
    if (c == 0) T.sy[(size_t)blockIdx.y * T.n_segments + i] = y;
}


// The pair sum of one piece of the plan's segments and one tile of pairs (heig_tile).  grid (piece, tile, column)
template <int CR>
__global__ void __launch_bounds__(256) hte_pair_kernel(PmlHteArgs T) {
    __shared__ double buf[CR * 64];   // the wavefronts' sums
    const PmlHeigArgs& A = T.h;
    const int k = A.k, ks = A.ks;
    const HeigTile t = heig_tile<CR>(A);
    double acc[CR];
#pragma unroll
    for (int j = 0; j < CR; ++j) acc[j] = 0.0;
    const int i0 = T.piece_off[blockIdx.x], i1 = T.piece_off[blockIdx.x + 1];
    for (int i = i0 + t.wave; i < i1; i += 4) {
        const double* st = T.sstage + ((size_t)blockIdx.z * T.n_segments + i) * 3 * ks;
        const double y = T.sy[(size_t)blockIdx.z * T.n_segments + i];
        const double E_d = st[t.dcl];
        const double r_d = t.d_in ? st[ks + t.dcl] : 0.0;
#pragma unroll
        for (int j = 0; j < CR; ++j) {
            const int c = t.c0 + j, cc = min(c, k - 1);   // (uniform over the wavefront)
            const double l_c = c < k ? st[2 * ks + cc] : 0.0;
            acc[j] += l_c * heig_Phi(y, t.ev[cc], t.ev_d, st[cc], E_d) * r_d;
            // (one pair's chain at a time, as the branches of heig_pair_kernel's per-branch sum leave it there: scheduled as one
            // block, the CR chains take 217 registers at CR = 32 -- two wavefronts per SIMD -- where this takes 157, three)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    heig_tile_sums<CR>(t, buf, acc, k, T.partial + ((size_t)blockIdx.z * T.n_pieces + blockIdx.x) * k * k);
}

// The kernels per bin below: grid (M ceil(k k / 256), column), the bin the slow index of x (pml_bin_entry), and heig's
// transforms on bin m's W.  W_m: the partials of bin m's pieces in piece order (an empty bin: exact zeros).
static __global__ void __launch_bounds__(256) hte_reduce_kernel(PmlHteArgs T) {
    const int k = T.h.k;
    int m, idx;
    if (!pml_bin_entry(k, m, idx)) return;
    T.Wsum[((size_t)blockIdx.y * T.M + m) * k * k + idx] =
        pml_piece_sum(T.partial + (size_t)blockIdx.y * T.n_pieces * k * k + idx, (size_t)k * k, T.bin_piece_off[m], T.bin_piece_off[m + 1]);
}

static __global__ void __launch_bounds__(256) hte_t1_kernel(PmlHteArgs T) {
    const int k = T.h.k;
    int m, idx;
    if (!pml_bin_entry(k, m, idx)) return;
    const size_t at = ((size_t)blockIdx.y * T.M + m) * k * k;
    heig_t1(T.h, blockIdx.y, idx, T.Wsum + at, T.T1 + at);
}

static __global__ void __launch_bounds__(256) hte_jumps_kernel(PmlHteArgs T) {
    const int k = T.h.k;
    int m, idx;
    if (!pml_bin_entry(k, m, idx)) return;
    const size_t at = ((size_t)blockIdx.y * T.M + m) * k * k;
    heig_jumps(T.h, blockIdx.y, idx, T.T1 + at, T.jumps_out + at);
}

// grid (M, column), thread s
static __global__ void __launch_bounds__(256) hte_times_kernel(PmlHteArgs T) {
    const int k = T.h.k;
    const size_t at = (size_t)blockIdx.y * T.M + blockIdx.x;
    if ((int)threadIdx.x < k) heig_times(T.h, blockIdx.y, threadIdx.x, T.T1 + at * k * k, T.times_out + at * k);
}
// The posterior of the state at the flagged segments' points, added up over one piece.  grid (piece, column), 256 threads,
// dynamic LDS: 16 (kp + 1) + 48 doubles and 16 ints, kp = k rounded up to 16; X[b][s] as in heig_basis_kernel.  Per tile of 16
// segments: X = l o e^{d s t'}, a = Ainv^T X; X = r o e^{d u t'}, b = A X; X = a o b (q_p where t' = 0); thread j adds X[.][j]
// in segment order.  Segments beyond the piece enter as zeros.
template <bool MFMA>
__global__ void __launch_bounds__(256) hte_lineage_kernel(PmlHteArgs T) {
    extern __shared__ double hte_lds[];
    constexpr int NR = MFMA ? 16 : 1;
    const PmlHeigArgs& A = T.h;
    const int k = A.k, ks = A.ks, kp = (k + 15) & ~15, LD = kp + 1;
    double* X = hte_lds;
    double* tb = hte_lds + 16 * LD;   // t' of the tile's segments; < 0: beyond the piece
    double* fs = tb + 16;             // s and u of the tile's segments
    double* fu = fs + 16;
    int* node = (int*)(fu + 16);      // caller's id
    const int col = A.col0 + blockIdx.y;
    const size_t colN = (size_t)col * A.N;
    const double* ev = A.ev + (size_t)col * k;
    const double* Am = A.A + (size_t)col * k * k;
    const double* Ai = A.Ainv + (size_t)col * k * k;
    const int i0 = T.lpiece_off[blockIdx.x], i1 = T.lpiece_off[blockIdx.x + 1];
    double acc = 0.0;
    for (int base = i0; base < i1; base += PML_HTE_TILE) {
        if (threadIdx.x < 16) {
            const int i = min(base + (int)threadIdx.x, i1 - 1);
            const int id = T.lin_node[i];
            node[threadIdx.x] = id;
            tb[threadIdx.x] = base + (int)threadIdx.x < i1 ? A.tprime[(size_t)blockIdx.y * A.N + id] : -1.0;
            fs[threadIdx.x] = T.lin_frac[4 * (size_t)i];
            fu[threadIdx.x] = T.lin_frac[4 * (size_t)i + 3];
        }
        __syncthreads();
        double a[NR], res[NR];
        // which: 2 = l with the fractions s, 1 = r with the fractions u
        auto fill = [&](int which, const double* f) {
            for (int e = threadIdx.x; e < 16 * kp; e += 256) {
                const int b = e / kp, s = e % kp, ss = min(s, k - 1);
                const double t = tb[b];
                const double x = A.stage[((size_t)blockIdx.y * A.N + node[b]) * 3 * ks + which * ks + ss];
                X[b * LD + s] = (s < k && t > 0.0) ? x * exp(ev[ss] * (f[b] * t)) : 0.0;
            }
        };
        fill(2, fs);
        __syncthreads();
        heig_product<MFMA>(Ai, true, X, k, a);
        __syncthreads();
        fill(1, fu);
        __syncthreads();
        heig_product<MFMA>(Am, false, X, k, res);
        __syncthreads();
#pragma unroll
        for (int idx = 0; idx < NR; ++idx) {
            int s, b;
            if (!heig_owned<MFMA>(idx, kp, s, b) || s >= k) continue;
            double x = a[idx] * res[idx];
            if (tb[b] == 0.0) {   // the formula at P = I
                const int n = A.new_of_old ? A.new_of_old[node[b]] : node[b];
                x = A.post[(colN + max(A.parent[n], 0)) * ks + s];
            }
            X[b * LD + s] = tb[b] < 0.0 ? 0.0 : x;
        }
        __syncthreads();
        if ((int)threadIdx.x < k)
            for (int b = 0; b < 16; ++b) acc += X[b * LD + threadIdx.x];
        __syncthreads();
    }
    if ((int)threadIdx.x < k) T.lpart[((size_t)blockIdx.y * T.n_lpieces + blockIdx.x) * k + threadIdx.x] = acc;
}

// lineages[m][j]: the pieces of boundary m in piece order, clamped at 0 (no flagged segment: exact zeros).  grid (M + 1, column)
static __global__ void __launch_bounds__(256) hte_lineage_sum_kernel(PmlHteArgs T) {
    const int k = T.h.k, j = threadIdx.x, m = blockIdx.x;
    if (j >= k) return;
    const double s = pml_piece_sum(T.lpart + (size_t)blockIdx.y * T.n_lpieces * k + j, k, T.bin_lpiece_off[m], T.bin_lpiece_off[m + 1]);
    T.lineages_out[((size_t)blockIdx.y * (T.M + 1) + m) * k + j] = s > 0.0 ? s : 0.0;
}

