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
// history_time_segment_kernel has history_branch_kernel's lane shapes and streams v_n and q_p once per segment; it leaves the
// pieces' partial times, sum x a and lineages, and stages S_n, x O C1b and x Cee per SEGMENT (C1b and Cee differ between the
// segments of one branch).  history_time_jump_kernel forms sum (x b) (x) v on the FP64 matrix cores, tiled as
// history_jump_kernel is; the two sum kernels add the partials in piece order per bin.
//
// Bits.  No floating-point atomics.  The plan sorts the segments by (bin, caller's id) and the pieces are cut PER BIN -- a
// fixed number of segments that depends on k only, never across a bin's end -- so a bin's sums see the same pieces in the same
// order whatever other bins the call has, and nothing depends on the grid, the schedule of the sweeps, the library's numbering
// or the column.
#pragma once
#include "pml_kernels_history.h"   // (hist_coefficients, hist_v, group_sum, PmlHistArgs)

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

// The segment pass.  G lanes per segment, R states per lane (state g + G r of lane g), 64 / G segments per wavefront, four
// wavefronts.  grid (piece, column).
template <int G, int R>
__global__ void __launch_bounds__(256) history_time_segment_kernel(PmlHistTimeArgs T) {
    constexpr int U = 64 / G, UNITS = 4 * U, ROW = 3 * G * R;
    __shared__ double red[UNITS * ROW];
    const PmlHistArgs& A = T.h;
    const int k = A.k, ks = A.ks;
    const int lane = threadIdx.x & 63, g = lane % G;
    const int unit = (threadIdx.x >> 6) * U + lane / G;
    const int col = A.col0 + blockIdx.y;
    const size_t colN = (size_t)col * A.N;
    const double mu = A.mu[col], tau = A.tau[col], tauf = A.tauf[col], scale = tauf * A.sf[col];
    double pi[R], acc_t[R], acc_a[R], acc_l[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int b = g + G * r;
        pi[r] = b < k ? A.pi[(size_t)col * ks + b] : 0.0;
        acc_t[r] = acc_a[r] = acc_l[r] = 0.0;
    }
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
        const int pp = max(A.parent[n], 0);   // (the plan holds no root)
        const bool tip = A.n_children[n] == 0;
        const size_t row = colN + n;
        const double e_stored = A.E[row];
        const double d = A.dist[n] + tau;
        const double x = inside ? mu * (d * scale) : 0.0;   // (the transform of f81_prep_kernel)
        const double len = inside ? d * tauf : 0.0;
        double v[R], q[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int b = g + G * r, bb = min(b, k - 1);
            const u64 m = A.masks[row * A.W + (bb >> 6)];
            const double x_bu = A.bu[row * ks + bb];
            const double y = A.post[(colN + pp) * ks + bb];
            const bool allowed = b < k && ((m >> (bb & 63)) & 1ull);
            v[r] = allowed ? (tip ? 1.0 : x_bu) : 0.0;
            q[r] = (inside && b < k) ? y : 0.0;
        }
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) s += pi[r] * v[r];
        s = group_sum<G>(s);
        const double rest = (1.0 - e_stored) * s;
        double o[R], o_sum = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double m = rest + e_stored * v[r];
            o[r] = (q[r] > 0.0 && m > 0.0) ? q[r] / m : 0.0;
            o_sum += o[r];
        }
        o_sum = group_sum<G>(o_sum);
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
            const double a = pi[r] * os0 + o[r] * sc1;
            const double b = pi[r] * oc1 + o[r] * Cee;
            acc_t[r] += len * (a + b * v[r]);
            acc_a[r] += x * a;
            acc_l[r] += (l_ov * o[r] * v[r] + l_o * o[r]) + (l_pv * pi[r] * v[r] + l_p * pi[r]);
        }
        if (g == 0 && inside && T.stage != nullptr) {
            double* st = T.stage + ((size_t)blockIdx.y * T.n_segments + i) * 3;
            st[0] = s;
            st[1] = x * oc1;
            st[2] = x * Cee;
        }
    }
    // the units' sums in unit order
    double* mine = red + unit * ROW;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        mine[g + G * r] = acc_t[r];
        mine[G * R + g + G * r] = acc_a[r];
        mine[2 * G * R + g + G * r] = acc_l[r];
    }
    __syncthreads();
    double* out = T.partial + ((size_t)blockIdx.y * T.n_pieces + blockIdx.x) * 3 * k;
    for (int t = threadIdx.x; t < 3 * k; t += 256) {
        const int which = t / k, at = which * G * R + (t - which * k);
        double sum = 0.0;
        for (int j = 0; j < UNITS; ++j) sum += red[j * ROW + at];
        out[t] = sum;
    }
}

// times, sum x a and lineages of one bin: its pieces' partials in piece order (an empty bin: exact zeros).  grid (M + 1,
// column); the pseudo-bin M gives the lineages at the last boundary only.  Thread t owns the entries t + 256 h of the 3 k.
static __global__ void __launch_bounds__(256) history_time_vector_kernel(PmlHistTimeArgs T) {
    const int k = T.h.k, M = T.M, m = blockIdx.x;
    const int p0 = T.bin_piece_off[m], p1 = T.bin_piece_off[m + 1];
    const double* part = T.partial + (size_t)blockIdx.y * T.n_pieces * 3 * k;
    for (int t = threadIdx.x; t < 3 * k; t += 256) {
        double s = 0.0;
        for (int j = p0; j < p1; ++j) s += part[(size_t)j * 3 * k + t];
        if (t < k) {
            if (m < M) T.times_out[((size_t)blockIdx.y * M + m) * k + t] = s;
        } else if (t < 2 * k) {
            if (m < M) T.xa[((size_t)blockIdx.y * M + m) * k + (t - k)] = s;
        } else if (T.lineages_out != nullptr) {
            T.lineages_out[((size_t)blockIdx.y * (M + 1) + m) * k + (t - 2 * k)] = s;
        }
    }
}

// sum (x b) (x) v over the segments of one piece.  grid (piece, tile group, column), tiled as history_jump_kernel: a wavefront
// owns the 16 rows i of one band and four bands of columns j; per step the four lane rows (hi) hold four consecutive segments:
// A[m][kk] = x b_kk[i0 + m], B[kk][n] = v_kk[j0 + n] (v_mfma_f64_16x16x4_f64; D: col = lane & 15, row = (lane >> 4) + 4 reg).
// States beyond k and segments beyond the piece enter as zeros.
// WIDE = 0: up to 64 states, one tile group, the loop over the steps unrolled by four (the loads of 16 segments in flight).
template <int WIDE>
__global__ void __launch_bounds__(256) history_time_jump_kernel(PmlHistTimeArgs T) {
    const PmlHistArgs& A = T.h;
    const int k = A.k, ks = A.ks;
    const int TT = (k + 15) >> 4, TG = WIDE ? (TT + 3) >> 2 : 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lo = lane & 15, hi = lane >> 4;
    const int ga = blockIdx.y / TG, gb = blockIdx.y % TG;
    const int ta = 4 * ga + wave;
    if (ta >= TT) return;   // (no barrier below)
    const int col = A.col0 + blockIdx.z;
    const size_t colN = (size_t)col * A.N;
    const int a = 16 * ta + lo;
    const double pi_a = a < k ? A.pi[(size_t)col * ks + a] : 0.0;
    pml_v4f64 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = pml_v4f64{0.0, 0.0, 0.0, 0.0};
    const int i0 = T.jpiece_off[blockIdx.x], i1 = T.jpiece_off[blockIdx.x + 1];
    const int a_c = min(a, k - 1);
    auto step = [&](int base) {
        // (segments beyond the piece read its last one and are zeroed by the selects below: no load waits for a test)
        const int i = min(base + hi, i1 - 1);
        const bool valid = base + hi < i1;
        const int id = T.seg_node[i];
        const int n = A.new_of_old ? A.new_of_old[id] : id;
        const int pp = max(A.parent[n], 0);
        const bool tip = A.n_children[n] == 0;
        const size_t row = colN + n;
        const double e_stored = A.E[row];
        const double q = A.post[(colN + pp) * ks + a_c];
        const double* st = T.stage + ((size_t)blockIdx.z * T.n_segments + i) * 3;
        const double S = st[0], xoc1 = st[1], xe = st[2];
        double w[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) w[t] = hist_v(A, row, tip, 16 * (4 * gb + t) + lo);
        double va = 0.0;
        if (!WIDE) {   // up to 64 states: the four tiles are the whole row
#pragma unroll
            for (int t = 0; t < 4; ++t) va = t == wave ? w[t] : va;
        } else {
            va = hist_v(A, row, tip, a);
        }
        const double m = (1.0 - e_stored) * S + e_stored * va;
        const double o = (valid && a < k && q > 0.0 && m > 0.0) ? q / m : 0.0;
        const double u = valid ? pi_a * xoc1 + o * xe : 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(u, valid ? w[t] : 0.0, acc[t], 0, 0, 0);
    };
    if (!WIDE) {
        // (by hand: the MFMA is convergent, which keeps the compiler from unrolling a loop with a remainder; steps beyond the
        // piece are all-zero operands)
        for (int base = i0; base < i1; base += 16) {
            step(base);
            step(base + 4);
            step(base + 8);
            step(base + 12);
        }
    } else {
        for (int base = i0; base < i1; base += 4) step(base);
    }
    double* out = T.jpartial + ((size_t)blockIdx.z * T.n_jpieces + blockIdx.x) * k * k;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int b = 16 * (4 * gb + t) + lo;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = 16 * ta + hi + 4 * reg;
            if (r < k && b < k) out[(size_t)r * k + b] = acc[t][reg];
        }
    }
}

// jumps[col][m][i][j] = pi_j (sum x a [m][i] + the products of bin m's pieces in piece order [i][j]), the diagonal 0.
// grid (M ceil(k k / 256), column): the bin is the slow index of x (M may exceed what y holds)
static __global__ void __launch_bounds__(256) history_time_matrix_kernel(PmlHistTimeArgs T) {
    const int k = T.h.k, M = T.M, per_bin = (k * k + 255) / 256;
    const int m = blockIdx.x / per_bin;
    const int idx = (blockIdx.x % per_bin) * 256 + threadIdx.x;
    if (idx >= k * k) return;
    const double* part = T.jpartial + (size_t)blockIdx.y * T.n_jpieces * k * k + idx;
    double s = 0.0;
    for (int j = T.bin_jpiece_off[m]; j < T.bin_jpiece_off[m + 1]; ++j) s += part[(size_t)j * k * k];
    const int i = idx / k, j = idx % k;
    const double pi_j = T.h.pi[(size_t)(T.h.col0 + blockIdx.y) * T.h.ks + j];
    const size_t at = (size_t)blockIdx.y * M + m;
    T.jumps_out[at * k * k + idx] = i == j ? 0.0 : pi_j * (T.xa[at * k + i] + s);
}
