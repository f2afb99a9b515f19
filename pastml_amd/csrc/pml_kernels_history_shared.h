// What the exact histories of the F81 family share: the whole-tree sums (pml_kernels_history.h) and the sums per time interval
// (pml_kernels_history_time.h) walk different items -- nodes there, segments of the plan here -- with different coefficients,
// and everything else is one body each: the arguments of a marginal pass, the coefficients' series, the clamped loads of v_n,
// the front half of the per-item pass, the units' sums through LDS, the jump product on the FP64 matrix cores and the sums of
// the pieces' partials.  No kernel lives here: a unit that includes this emits what it launches and nothing else.
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

// ---- the per-item pass: history_branch_kernel (items: the ids of a piece) and history_time_segment_kernel (the segments of
// a piece).  gradient_f81_kernel's lane shapes: G lanes per item, R states per lane (state g + G r of lane g), 64 / G items
// per wavefront, four wavefronts; a unit is the G lanes of one item.

// What a lane keeps of its column: the parameters and the frequencies of its R states (0 beyond k)
template <int R>
struct HistColumn {
    size_t colN;
    double mu, tau, tauf, scale, pi[R];
};
template <int G, int R>
__device__ __forceinline__ HistColumn<R> hist_column(const PmlHistArgs& A, int col, int g) {
    HistColumn<R> C;
    C.colN = (size_t)col * A.N;
    C.mu = A.mu[col], C.tau = A.tau[col], C.tauf = A.tauf[col], C.scale = C.tauf * A.sf[col];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int b = g + G * r;
        C.pi[r] = b < A.k ? A.pi[(size_t)col * A.ks + b] : 0.0;
    }
    return C;
}

// The front half for node n with parent p (a root: any; it reads parent 0): v = v_n, s = S_n = pi . v_n, o = o_n and
// o_sum = O_n; o is 0 throughout where the item does not add.  No load waits for a test (hist_v's rule; the posterior of the
// parent likewise), and the two sums over the unit's lanes are convergent.
template <int G, int R>
__device__ __forceinline__ void hist_front(const PmlHistArgs& A, const HistColumn<R>& C, int g, int n, int p, bool adds, double (&v)[R],
                                           double (&o)[R], double& s, double& o_sum) {
    const int k = A.k, ks = A.ks;
    const int pp = max(p, 0);
    const bool tip = A.n_children[n] == 0;
    const size_t row = C.colN + n;
    const double e_stored = A.E[row];
    double q[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int b = g + G * r, bb = min(b, k - 1);
        const u64 m = A.masks[row * A.W + (bb >> 6)];
        const double x_bu = A.bu[row * ks + bb];
        const double y = A.post[(C.colN + pp) * ks + bb];
        const bool allowed = b < k && ((m >> (bb & 63)) & 1ull);
        v[r] = allowed ? (tip ? 1.0 : x_bu) : 0.0;
        q[r] = (adds && b < k) ? y : 0.0;
    }
    s = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) s += C.pi[r] * v[r];
    s = group_sum<G>(s);
    const double rest = (1.0 - e_stored) * s;
    o_sum = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double m = rest + e_stored * v[r];
        o[r] = (q[r] > 0.0 && m > 0.0) ? q[r] / m : 0.0;
        o_sum += o[r];
    }
    o_sum = group_sum<G>(o_sum);
}

// The units' sums in unit order: B blocks of k entries each (acc: one double [R] per block, entry g + G r of the block),
// through red [4 (64 / G)][B G R] in LDS, into out [B k].  Every thread of the workgroup comes here.
// (The blocks are arrays of their own, not one [B][R]: with one array history_time_segment_kernel<64, 8> takes 256 registers
// and ten more as AGPRs, one wavefront per SIMD, against 248 and two.)
template <int G, int R, class... Acc>
__device__ __forceinline__ void hist_unit_sums(double* red, int unit, int g, int k, double* out, const Acc&... acc) {
    constexpr int B = sizeof...(Acc), UNITS = 4 * (64 / G), ROW = B * G * R;
    double* mine = red + unit * ROW;
    auto put = [&](const double (&block)[R]) {
#pragma unroll
        for (int r = 0; r < R; ++r) mine[g + G * r] = block[r];
        mine += G * R;
    };
    (put(acc), ...);
    __syncthreads();
    for (int t = threadIdx.x; t < B * k; t += 256) {
        const int which = t / k, at = which * G * R + (t - which * k);
        double sum = 0.0;
        for (int j = 0; j < UNITS; ++j) sum += red[j * ROW + at];
        out[t] = sum;
    }
}

// ---- the sums of the pieces' partials

// One entry over the pieces [p0, p1) in piece order (none: an exact zero); part: the entry in piece 0, stride: doubles per piece
__device__ __forceinline__ double pml_piece_sum(const double* part, size_t stride, int p0, int p1) {
    double s = 0.0;
    for (int j = p0; j < p1; ++j) s += part[(size_t)j * stride];
    return s;
}

// Entry idx = i k + j of a jumps matrix: pi_j (sum x a [i] + the products of the pieces [p0, p1) in piece order [i][j]), the
// diagonal 0.  column: the grid's; jpartial: the column's pieces; xa: the k sums the matrix belongs to.
__device__ __forceinline__ double hist_jumps_entry(const PmlHistArgs& A, int column, int idx, const double* jpartial, int p0, int p1,
                                                   const double* xa) {
    const int k = A.k;
    const double s = pml_piece_sum(jpartial + idx, (size_t)k * k, p0, p1);
    const int i = idx / k, j = idx % k;
    const double pi_j = A.pi[(size_t)(A.col0 + column) * A.ks + j];
    return i == j ? 0.0 : pi_j * (xa[i] + s);
}

// A grid over (bin, k k entries), the bin the slow index of blockIdx.x (M may exceed what y holds): this thread's bin m and
// entry idx; false beyond the k k
__device__ __forceinline__ bool pml_bin_entry(int k, int& m, int& idx) {
    const int per_bin = (k * k + 255) / 256;
    m = blockIdx.x / per_bin;
    idx = (blockIdx.x % per_bin) * 256 + threadIdx.x;
    return idx < k * k;
}

// ---- the jump product: sum (x b) (x) v over the items [i0, i1) of one piece, into out [k][k].  grid (piece, tile group,
// column), tiled as expected_f81_kernel: a wavefront owns the 16 rows i of one band and four bands of columns j; per step the
// four lane rows (hi) hold four consecutive items: A[m][kk] = x b_kk[i0 + m], B[kk][n] = v_kk[j0 + n]
// (v_mfma_f64_16x16x4_f64; D: col = lane & 15, row = (lane >> 4) + 4 reg).  States beyond k and items that do not add enter
// as zeros.  WIDE = 0: up to 64 states, one tile group, the loop over the steps unrolled by four (the loads of 16 items in
// flight).
// items.at(i, n, stage_row): the node of item i (library's numbering) and the row of its three staged scalars S, x O c1, x e in
// stage, the column's [rows][3]; items.valid(inside, p): whether an item inside the piece whose node has parent p adds.
template <int WIDE, class Items>
__device__ __forceinline__ void hist_jump_product(const PmlHistArgs& A, const Items& items, const double* stage, int i0, int i1,
                                                  double* out) {
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
    const int a_c = min(a, k - 1);
    auto step = [&](int base) {
        // (items beyond the piece read its last one, roots parent 0, and are zeroed by the selects below: no load waits for a test)
        const int i = min(base + hi, i1 - 1);
        int n, stage_row;
        items.at(i, n, stage_row);
        const int p = A.parent[n];
        const bool valid = items.valid(base + hi < i1, p);
        const int pp = max(p, 0);
        const bool tip = A.n_children[n] == 0;
        const size_t row = colN + n;
        const double e_stored = A.E[row];
        const double q = A.post[(colN + pp) * ks + a_c];
        const double* st = stage + (size_t)stage_row * 3;
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
