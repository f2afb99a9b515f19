// Exact expected dwell times, Markov jumps and lineage counts per time interval for the F81 family, all columns of a call in one
// pass (pml_history_through_time): pml_kernels_history.h's sums with every branch cut at the boundaries of the time bins.
//
// The host plans the cut (pml_time_segments.h): a segment is the part [s1, s1 + w] of a branch n, as fractions of the branch,
// that lies in one bin; r = 1 - s1 - w is what is left below it.  In the notation of pml_kernels_history.h, with y = w x_n,
// (e_y, c0_y, c1_y) = hist_coefficients(y), A = -expm1(-s1 x_n), B = -expm1(-r x_n):
//     C0  = w (c0_y + (A + B) c1_y + A B e_y)        C1a = w (1 - A) (c1_y + B e_y)
//     C1b = w (1 - B) (c1_y + A e_y)                 Cee = w (1 - A) (1 - B) e_y                 (C0 + C1a + C1b + Cee = w)
//     a[i] = pi_i O S C0 + o_i S C1a,   b[i] = pi_i O C1b + o_i Cee
//     times[m][s]    += L_n (a[s] + b[s] v_n[s])
//     jumps[m][i][j] += x_n pi_j (a[i] + b[i] v_n[j])      (i != j)
// (the integrals of alpha_i(s) beta_j(s) over the segment: alpha the state at s given the parent's side, beta given the
// child's).  A segment whose branch is alive at the boundary its bin begins with (flagged by the plan) also adds, with
// A = -expm1(-s1 x), B = -expm1(-u x), u = 1 - s1 as the plan formed it, the posterior of the state at that point,
//     lineages[m][j] += (1-A)(1-B) o_j v_j + (1-A) B o_j S + A (1-B) pi_j O v_j + A B pi_j O S            (sums to 1 over j)
// Every term is non-negative.  The zero-width point segments of the last boundary (pseudo-bin M) add lineages only: w = 0.
//
// history_time_segment_kernel has history_branch_kernel's lane shapes and front half (hist_front) and streams v_n and q_p
// once per segment; it leaves the pieces' partial times, sum x a and lineages, and stages S_n, x O C1b and x Cee per SEGMENT
// (C1b and Cee differ between the segments of one branch).  history_time_jump_kernel forms sum (x b) (x) v on the FP64 matrix
// cores (hist_jump_product); the two sum kernels add the partials in piece order per bin.  What is shared with the whole-tree
// sums is pml_kernels_history_shared.h's; none of pml_kernels_history.h's kernels is seen here.
//
// Bits.  No floating-point atomics.  The plan sorts the segments by (bin, caller's id) and the pieces are cut PER BIN -- a
// fixed number of segments that depends on k only, never across a bin's end -- so a bin's sums see the same pieces in the same
// order whatever other bins the call has, and nothing depends on the grid, the schedule of the sweeps, the library's numbering
// or the column.
#pragma once
#include "pml_kernels_history_shared.h"

struct PmlHistTimeArgs {
    PmlHistArgs h;                  // the vectors of the marginal pass, the parameters, N, k, ks, W, col0 (hist_v reads it)
    int M;                          // time bins
    int n_segments;                 // all segments, the point segments of the pseudo-bin M included
    const int* seg_node;            // [n_segments] caller's id
    const int* seg_starts;          // [n_segments] 1: adds to the lineages of its bin's boundary
    const double* seg_frac;         // [n_segments][4]: s1, w, r, u
    const int* piece_off;           // [n_pieces + 1] segment pass: the pieces of all bins and of the pseudo-bin
    const int* bin_piece_off;       // [M + 2]
    const int* jpiece_off;          // [n_jpieces + 1] jump product: the pieces of the bins 0 .. M - 1
    const int* bin_jpiece_off;      // [M + 1]
    int n_pieces, n_jpieces;
    double* partial;                // [cols][n_pieces][3 k]: times, sum x a, lineages
    double* stage;                  // [cols][n_segments][3]: S_n, x O C1b, x Cee; null without jumps
    double* jpartial;               // [cols][n_jpieces][k][k]
    double* xa;                     // [cols][M][k]
    double* times_out;              // [cols][M][k]
    double* jumps_out;              // [cols][M][k][k], or null
    double* lineages_out;           // [cols][M + 1][k], or null
};

// The segment pass (the lane shapes: pml_kernels_history_shared.h).  grid (piece, column).
template <int G, int R>
__global__ void __launch_bounds__(256) history_time_segment_kernel(PmlHistTimeArgs T) {
    constexpr int U = 64 / G, UNITS = 4 * U;
    __shared__ double red[UNITS * 3 * G * R];
    const PmlHistArgs& A = T.h;
    const int lane = threadIdx.x & 63, g = lane % G;
    const int unit = (threadIdx.x >> 6) * U + lane / G;
    const HistColumn<R> C = hist_column<G, R>(A, A.col0 + blockIdx.y, g);
    double acc_t[R], acc_a[R], acc_l[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc_t[r] = acc_a[r] = acc_l[r] = 0.0;
    const int i0 = T.piece_off[blockIdx.x], i1 = T.piece_off[blockIdx.x + 1];   // (a piece holds one segment at least)
    for (int base = i0; base < i1; base += UNITS) {   // (the same trip count in every unit: the lane exchanges below are convergent)
        // (units beyond the piece read its last segment and are zeroed by the selects below: no load waits for a test)
        const int i = min(base + unit, i1 - 1);
        const bool inside = base + unit < i1;
        const int id = T.seg_node[i];
        const bool starts = inside && T.seg_starts[i] != 0;
        const double s1 = T.seg_frac[4 * (size_t)i], w = T.seg_frac[4 * (size_t)i + 1], rr = T.seg_frac[4 * (size_t)i + 2],
                     u = T.seg_frac[4 * (size_t)i + 3];
        const int n = A.new_of_old ? A.new_of_old[id] : id;
        const double d = A.dist[n] + C.tau;
        const double x = inside ? C.mu * (d * C.scale) : 0.0;   // (the transform of f81_prep_kernel)
        const double len = inside ? d * C.tauf : 0.0;
        double v[R], o[R], s, o_sum;
        hist_front<G, R>(A, C, g, n, A.parent[n], inside, v, o, s, o_sum);   // (the plan holds no root)
        double ey, c0y, c1y;
        hist_coefficients(w * x, ey, c0y, c1y);
        const double Aa = -expm1(-s1 * x), Bb = -expm1(-rr * x), Bl = -expm1(-u * x);
        const double C0 = w * (c0y + (Aa + Bb) * c1y + Aa * Bb * ey);
        const double C1a = w * (1.0 - Aa) * (c1y + Bb * ey);
        const double C1b = w * (1.0 - Bb) * (c1y + Aa * ey);
        const double Cee = w * (1.0 - Aa) * (1.0 - Bb) * ey;
        const double os0 = o_sum * s * C0, sc1 = s * C1a, oc1 = o_sum * C1b;
        // the point s1 of the branch: (1-A)(1-B) o v + (1-A) B o S + A (1-B) pi O v + A B pi O S
        const double l_ov = starts ? (1.0 - Aa) * (1.0 - Bl) : 0.0, l_o = starts ? (1.0 - Aa) * Bl * s : 0.0;
        const double l_pv = starts ? Aa * (1.0 - Bl) * o_sum : 0.0, l_p = starts ? Aa * Bl * o_sum * s : 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double a = C.pi[r] * os0 + o[r] * sc1;
            const double b = C.pi[r] * oc1 + o[r] * Cee;
            acc_t[r] += len * (a + b * v[r]);
            acc_a[r] += x * a;
            acc_l[r] += (l_ov * o[r] * v[r] + l_o * o[r]) + (l_pv * C.pi[r] * v[r] + l_p * C.pi[r]);
        }
        if (g == 0 && inside && T.stage != nullptr) {
            double* st = T.stage + ((size_t)blockIdx.y * T.n_segments + i) * 3;
            st[0] = s;
            st[1] = x * oc1;
            st[2] = x * Cee;
        }
    }
    hist_unit_sums<G, R>(red, unit, g, A.k, T.partial + ((size_t)blockIdx.y * T.n_pieces + blockIdx.x) * 3 * A.k, acc_t, acc_a, acc_l);
}

// times, sum x a and lineages of one bin: its pieces' partials in piece order (an empty bin: exact zeros).  grid (M + 1,
// column); the pseudo-bin M gives the lineages at the last boundary only.  Thread t owns the entries t + 256 h of the 3 k.
static __global__ void __launch_bounds__(256) history_time_vector_kernel(PmlHistTimeArgs T) {
    const int k = T.h.k, M = T.M, m = blockIdx.x;
    const double* part = T.partial + (size_t)blockIdx.y * T.n_pieces * 3 * k;
    for (int t = threadIdx.x; t < 3 * k; t += 256) {
        const double s = pml_piece_sum(part + t, (size_t)3 * k, T.bin_piece_off[m], T.bin_piece_off[m + 1]);
        if (t < k) {
            if (m < M) T.times_out[((size_t)blockIdx.y * M + m) * k + t] = s;
        } else if (t < 2 * k) {
            if (m < M) T.xa[((size_t)blockIdx.y * M + m) * k + (t - k)] = s;
        } else if (T.lineages_out != nullptr) {
            T.lineages_out[((size_t)blockIdx.y * (M + 1) + m) * k + (t - 2 * k)] = s;
        }
    }
}

// sum (x b) (x) v over the segments of one piece of the plan: item i is segment i, on the node with the caller's id
// seg_node[i]; its staged scalars are kept by segment, and the plan holds no root.  grid (piece, tile group, column)
struct HistSegmentItems {
    const int *seg_node, *new_of_old;
    __device__ __forceinline__ void at(int i, int& n, int& stage_row) const {
        const int id = seg_node[i];
        n = new_of_old ? new_of_old[id] : id;
        stage_row = i;
    }
    __device__ __forceinline__ bool valid(bool inside, int) const { return inside; }
};
template <int WIDE>
__global__ void __launch_bounds__(256) history_time_jump_kernel(PmlHistTimeArgs T) {
    hist_jump_product<WIDE>(T.h, HistSegmentItems{T.seg_node, T.h.new_of_old}, T.stage + (size_t)blockIdx.z * T.n_segments * 3,
                            T.jpiece_off[blockIdx.x], T.jpiece_off[blockIdx.x + 1],
                            T.jpartial + ((size_t)blockIdx.z * T.n_jpieces + blockIdx.x) * T.h.k * T.h.k);
}

// jumps[col][m][i][j]: hist_jumps_entry over bin m's pieces and its sum x a.  grid (M ceil(k k / 256), column)
static __global__ void __launch_bounds__(256) history_time_matrix_kernel(PmlHistTimeArgs T) {
    const int k = T.h.k;
    int m, idx;
    if (!pml_bin_entry(k, m, idx)) return;
    const size_t at = (size_t)blockIdx.y * T.M + m;
    T.jumps_out[at * k * k + idx] = hist_jumps_entry(T.h, blockIdx.y, idx, T.jpartial + (size_t)blockIdx.y * T.n_jpieces * k * k,
                                                     T.bin_jpiece_off[m], T.bin_jpiece_off[m + 1], T.xa + at * k);
}
