// Exact expected dwell times and Markov jumps along the tree for the F81 family (F81 / JC / EFT), all columns of a call in one
// pass (pml_expected_history): the posterior mean, over whole histories, of the time spent in each state and of the number of
// jumps i -> j -- events, not end-point differences (pml_kernels_expected.h counts those).
//
// Per column and non-root node n with parent p, in the notation of pml_kernels_gradient.h: mu = 1 / (1 - pi . pi),
// t'_n = (d_n + tau) tf sf, L_n = (d_n + tau) tf, x_n = mu t'_n, e_n = exp(-x_n), v_n the bottom-up vector of n (a tip: its 0/1
// mask; any scaling cancels), S_n = pi . v_n, m_n[i] = (1 - e_n) S_n + e_n v_n[i], q_p the marginal posterior of p,
// o_n[i] = q_p[i] / m_n[i] (0 where q_p[i] == 0), O_n = sum_i o_n[i].  With
//     g = (1 - e) / x,   c0 = 1 - 2 g + e,   c1 = g - e                                (all >= 0; g = 1, c0 = c1 = 0 at x = 0)
//     a_n[i] = pi_i O_n S_n c0 + o_n[i] S_n c1,     b_n[i] = pi_i O_n c1 + o_n[i] e_n
// the posterior share of branch n spent in state s is f_n[s] = a_n[s] + b_n[s] v_n[s] (sum_s f_n[s] = 1), the expected number
// of jumps i -> j on it is J_n[i][j] = x_n pi_j (a_n[i] + b_n[i] v_n[j]) for i != j, and
//     times[s]        = sum_n L_n f_n[s]
//     jumps[i][j]     = pi_j (sum_n x_n a_n[i]  +  sum_n x_n b_n[i] v_n[j])             (i != j; the diagonal is 0)
//     branch_jumps[n] = x_n sum_i (a_n[i] (1 - pi_i) + b_n[i] (S_n - pi_i v_n[i]))      (= sum_{i != j} J_n[i][j]; a root: 0)
// Every term is non-negative.  A branch with t' = 0 adds nothing.
//
// history_branch_kernel streams v_n and q_p once per branch (2 k doubles, as gradient_f81_kernel does) and leaves the pieces'
// partial times and sum x a; history_jump_kernel forms sum_n (x_n b_n) (x) v_n on the FP64 matrix cores, tiled as
// expected_f81_kernel is; history_vector_kernel and history_matrix_kernel sum the partials in piece order.
//
// b_n in the product.  It is formed again there, not staged: the branch pass leaves three doubles per branch and column -- S_n,
// x_n O_n c1 and x_n e_n, 24 bytes written and read once per tile group -- and the product forms
// x_n b_n[i] = pi_i (x_n O_n c1) + o_n[i] (x_n e_n) from the q_p and v_n it streams anyway (one division per element, no
// exponential).  Staging x_n b_n itself would be 8 k bytes per branch and column written and read: half as much again as the
// 16 k bytes the branch pass streams.
//
// 1 - e and e.  In m_n it is 1.0 - e_n with the stored e_n, as the sweeps formed it: q_p carries m_n as a factor, and
// q_p[i] / m_n[i] is that factor cancelled only if both are the same number (pml_kernels_gradient.h).  The explicit e_n, g, c0
// and c1 are formed from x_n: for x < 1 by  c1 = e sum_{m >= 1} x^m / (m + 1)!,  c0 = e sum_{m >= 2} x^m (m - 1) / (m + 1)!
// (the series of the header times e^x e^-x: every term positive, no cancellation; 1 - 2 g + e formed directly has no digit left
// at x = 1e-9), from expm1 otherwise.
//
// Bits.  No floating-point atomics.  The nodes are walked in the CALLER's numbering and cut into pieces of a fixed number of
// ids (a function of k only, one size for the branch pass and one for the product); a workgroup owns one piece (and tile
// group), the units of the branch pass take the ids of the piece round robin and their sums are combined through LDS in unit
// order, and the partials are summed in piece order.  Nothing depends on the grid, on the schedule of the sweeps, on the
// library's own numbering or on the column.
#pragma once
#include "pml_kernels_pij.h"   // (pml_v4f64)

struct PmlHistArgs {
    const int* parent;              // the library's numbering, as all per-node arrays below
    const int* n_children;
    const int* new_of_old;          // caller's id -> library's id; null = the same
    const double* dist;             // [N]
    const u64* masks;               // [C][N][W]
    const double* pi;               // [C][ks]
    const double* bu;               // [C][N][ks]   (tips: not stored, their masks as 0/1)
    const double* post;             // [C][N][ks]
    const double* E;                // [C][N]
    const double *mu, *sf, *tau, *tauf;   // [C]
    int N, k, ks, W;
    int col0;                       // first column of the call; the grid's column index counts from it
    int piece, n_pieces;            // ids per piece of the branch pass
    int jpiece, n_jpieces;          // ids per piece of the jump product
    double* partial;                // [cols][n_pieces][2 k]: times[0..k), sum x a [0..k)
    double* stage;                  // [cols][N][3] (library's numbering): S_n, x_n O_n c1, x_n e_n; null without jumps
    double* jpartial;               // [cols][n_jpieces][k][k]: sum x b (x) v
    double* xa;                     // [cols][k]: sum_n x_n a_n
    double* times_out;              // [cols][k]
    double* branch_out;             // [cols][N] caller's numbering, or null
    double* jumps_out;              // [cols][k][k], or null
};

#define PML_HIST_TERMS 20
struct HistSeries {
    double inv[PML_HIST_TERMS + 1];   // 1 / (m + 1)!
};
constexpr HistSeries hist_series_table() {
    HistSeries t{};
    double f = 1.0;   // (m + 1)!: exact in a double up to 21!
    for (int m = 1; m <= PML_HIST_TERMS; ++m) {
        f *= (double)(m + 1);
        t.inv[m] = 1.0 / f;
    }
    return t;
}

// e = exp(-x), c0 = 1 - 2 g + e, c1 = g - e with g = (1 - e) / x, for x >= 0.  Below 1 the positive series (the term of x^20 is
// under 1e-17 of the first one), both from the one table: with U_m = sum_{j >= m} x^(j - m) / (j + 1)! (Horner's partial sums)
// c1 = e x U_1, and sum_{m >= 2} (m - 1) t_m is the sum of the tails sum_{j >= m} t_j = x^m U_m over m >= 2, a second Horner
// sum over the U_m.  From 1 on the closed forms lose one digit at most (c0(1) = 0.104 from terms of size 1; 1 - e >= 0.63).
__device__ __forceinline__ void hist_coefficients(double x, double& e, double& c0, double& c1) {
    constexpr HistSeries T = hist_series_table();
    e = exp(-x);
    if (x < 1.0) {
        double U = 0.0, V = 0.0;
#pragma unroll
        for (int m = PML_HIST_TERMS; m >= 2; --m) {
            U = fma(U, x, T.inv[m]);
            V = fma(V, x, U);
        }
        U = fma(U, x, T.inv[1]);
        c1 = e * (U * x);
        c0 = e * (V * (x * x));
    } else {
        const double g = (1.0 - e) / x;
        c0 = (1.0 - 2.0 * g) + e;
        c1 = g - e;
    }
}

// v_n[b]: the bottom-up entry, a tip's mask as 0/1, 0 where the mask excludes b or b >= k; row = col * N + n.  Every load is
// issued whatever the mask, the tip flag or b say (a clamped address, a select afterwards), as exp_weight does.
__device__ __forceinline__ double hist_v(const PmlHistArgs& A, size_t row, bool tip, int b) {
    const int bb = min(b, A.k - 1);
    const u64 m = A.masks[row * A.W + (bb >> 6)];
    const double x = A.bu[row * A.ks + bb];
    const bool allowed = b < A.k && ((m >> (bb & 63)) & 1ull);
    return allowed ? (tip ? 1.0 : x) : 0.0;
}

// The branch pass: gradient_f81_kernel's lane shapes.  G lanes per branch, R states per lane (state g + G r of lane g), 64 / G
// branches per wavefront, four wavefronts.  grid (piece, column).
template <int G, int R>
__global__ void __launch_bounds__(256) history_branch_kernel(PmlHistArgs A) {
    constexpr int U = 64 / G, UNITS = 4 * U, ROW = 2 * G * R;
    __shared__ double red[UNITS * ROW];
    const int k = A.k, ks = A.ks;
    const int lane = threadIdx.x & 63, g = lane % G;
    const int unit = (threadIdx.x >> 6) * U + lane / G;
    const int col = A.col0 + blockIdx.y;
    const size_t colN = (size_t)col * A.N;
    const double mu = A.mu[col], tau = A.tau[col], tauf = A.tauf[col], scale = tauf * A.sf[col];
    double pi[R], acc_t[R], acc_a[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int b = g + G * r;
        pi[r] = b < k ? A.pi[(size_t)col * ks + b] : 0.0;
        acc_t[r] = acc_a[r] = 0.0;
    }
    const int i0 = blockIdx.x * A.piece, i1 = min(A.N, i0 + A.piece);
    for (int base = i0; base < i1; base += UNITS) {   // (the same trip count in every unit: the lane exchanges below are convergent)
        const int i = min(base + unit, i1 - 1);
        const bool inside = base + unit < i1;
        const int n = A.new_of_old ? A.new_of_old[i] : i;
        const int p = A.parent[n];
        const int pp = max(p, 0);
        const bool tip = A.n_children[n] == 0;
        const bool branch = inside && p >= 0;
        const size_t row = colN + n;
        const double e_stored = A.E[row];
        const double d = A.dist[n] + tau;
        const double x = branch ? mu * (d * scale) : 0.0;   // (the transform of f81_prep_kernel)
        const double len = branch ? d * tauf : 0.0;
        double v[R], q[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int b = g + G * r, bb = min(b, k - 1);
            const u64 m = A.masks[row * A.W + (bb >> 6)];
            const double x_bu = A.bu[row * ks + bb];
            const double y = A.post[(colN + pp) * ks + bb];
            const bool allowed = b < k && ((m >> (bb & 63)) & 1ull);
            v[r] = allowed ? (tip ? 1.0 : x_bu) : 0.0;
            q[r] = (branch && b < k) ? y : 0.0;
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
        double e, c0, c1;
        hist_coefficients(x, e, c0, c1);
        const double os0 = o_sum * s * c0, sc1 = s * c1, oc1 = o_sum * c1;
        double bj = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double a = pi[r] * os0 + o[r] * sc1;
            const double b = pi[r] * oc1 + o[r] * e;
            acc_t[r] += len * (a + b * v[r]);
            acc_a[r] += x * a;
            bj += a * (1.0 - pi[r]) + b * (s - pi[r] * v[r]);
        }
        bj = group_sum<G>(bj);
        if (g == 0 && inside) {
            if (A.branch_out != nullptr) A.branch_out[(size_t)blockIdx.y * A.N + i] = x * bj;
            if (A.stage != nullptr) {
                double* st = A.stage + ((size_t)blockIdx.y * A.N + n) * 3;
                st[0] = s;
                st[1] = x * oc1;
                st[2] = x * e;
            }
        }
    }
    // the units' sums in unit order
    double* mine = red + unit * ROW;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        mine[g + G * r] = acc_t[r];
        mine[G * R + g + G * r] = acc_a[r];
    }
    __syncthreads();
    double* out = A.partial + ((size_t)blockIdx.y * A.n_pieces + blockIdx.x) * 2 * k;
    for (int t = threadIdx.x; t < 2 * k; t += 256) {
        const int at = t < k ? t : G * R + (t - k);
        double sum = 0.0;
        for (int j = 0; j < UNITS; ++j) sum += red[j * ROW + at];
        out[t] = sum;
    }
}

// times and sum x a: the pieces' partials in piece order.  grid (column); thread t owns the entries t + 256 h of the 2 k <= 1024.
static __global__ void __launch_bounds__(256) history_vector_kernel(PmlHistArgs A) {
    const int k = A.k;
    const double* part = A.partial + (size_t)blockIdx.x * A.n_pieces * 2 * k;
    for (int t = threadIdx.x; t < 2 * k; t += 256) {
        double s = 0.0;
        for (int j = 0; j < A.n_pieces; ++j) s += part[(size_t)j * 2 * k + t];
        if (t < k) A.times_out[(size_t)blockIdx.x * k + t] = s;
        else A.xa[(size_t)blockIdx.x * k + (t - k)] = s;
    }
}

// sum_n (x_n b_n) (x) v_n of one piece.  grid (piece, tile group, column), tiled as expected_f81_kernel: a wavefront owns the 16
// rows i of one band and four bands of columns j; per step the four lane rows (hi) hold four consecutive branches:
// A[m][kk] = x b_kk[i0 + m], B[kk][n] = v_kk[j0 + n] (v_mfma_f64_16x16x4_f64; D: col = lane & 15, row = (lane >> 4) + 4 reg).
// States beyond k and ids that are roots or beyond the piece enter as zeros.
// WIDE = 0: up to 64 states, one tile group, the loop over the steps unrolled by four (the loads of 16 branches in flight).
template <int WIDE>
__global__ void __launch_bounds__(256) history_jump_kernel(PmlHistArgs A) {
    const int k = A.k, ks = A.ks;
    const int T = (k + 15) >> 4, TG = WIDE ? (T + 3) >> 2 : 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lo = lane & 15, hi = lane >> 4;
    const int ga = blockIdx.y / TG, gb = blockIdx.y % TG;
    const int ta = 4 * ga + wave;
    if (ta >= T) return;   // (no barrier below)
    const int col = A.col0 + blockIdx.z;
    const size_t colN = (size_t)col * A.N;
    const int a = 16 * ta + lo;
    const double pi_a = a < k ? A.pi[(size_t)col * ks + a] : 0.0;
    pml_v4f64 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = pml_v4f64{0.0, 0.0, 0.0, 0.0};
    const int i0 = blockIdx.x * A.jpiece, i1 = min(A.N, i0 + A.jpiece);
    const int a_c = min(a, k - 1);
    auto step = [&](int base) {
        // (ids beyond the piece and roots read node 0 / parent 0 and are zeroed by the selects below: no load waits for a test)
        const int i = min(base + hi, i1 - 1);
        const int n = A.new_of_old ? A.new_of_old[i] : i;
        const int p = A.parent[n];
        const bool valid = base + hi < i1 && p >= 0;
        const int pp = max(p, 0);
        const bool tip = A.n_children[n] == 0;
        const size_t row = colN + n;
        const double e_stored = A.E[row];
        const double q = A.post[(colN + pp) * ks + a_c];
        const double* st = A.stage + ((size_t)blockIdx.z * A.N + n) * 3;
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
    double* out = A.jpartial + ((size_t)blockIdx.z * A.n_jpieces + blockIdx.x) * k * k;
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

// jumps[col][i][j] = pi_j (sum x a [i] + the pieces' products in piece order [i][j]), the diagonal 0.  grid (k k / 256, column)
static __global__ void __launch_bounds__(256) history_matrix_kernel(PmlHistArgs A) {
    const int k = A.k;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= k * k) return;
    const double* part = A.jpartial + (size_t)blockIdx.y * A.n_jpieces * k * k + idx;
    double s = 0.0;
    for (int j = 0; j < A.n_jpieces; ++j) s += part[(size_t)j * k * k];
    const int i = idx / k, j = idx % k;
    const double pi_j = A.pi[(size_t)(A.col0 + blockIdx.y) * A.ks + j];
    A.jumps_out[(size_t)blockIdx.y * k * k + idx] = i == j ? 0.0 : pi_j * (A.xa[(size_t)blockIdx.y * k + i] + s);
}
