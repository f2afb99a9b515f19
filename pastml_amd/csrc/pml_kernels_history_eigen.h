// Exact expected dwell times and Markov jumps along the tree for the eigen-decomposed models (JTT, CUSTOM_RATES, HKY handed over
// as an eigen model), all columns of a call in one pass (pml_expected_history_eigen): what pml_kernels_history.h computes for the
// F81 family, by the eigenbasis integral of Minin & Suchard / Hobolth & Jensen.  No P(t): memory is O(N k).
//
// Per column, with d[k], A[k][k], Ainv[k][k] the doubles of pml_model_set_eigen, Q = A diag(d) Ainv, t'_n = (dist_n + tau) tf sf,
// L_n = t'_n / sf, and for every non-root node n with parent p and t'_n > 0:
//     v_n     bottom-up vector of n (a tip: its 0/1 mask; any scaling cancels)
//     r_n   = Ainv v_n,   E_n = exp(d t'_n),   m_n = A (E_n o r_n)   (= P(t'_n) v_n)
//     o_n[a]= q_p[a] / m_n[a]   (0 where q_p[a] == 0), q_p the marginal posterior of p,      l_n = A^T o_n
//     Phi_cd(t) = integral_0^t exp(d_c u) exp(d_d (t - u)) du = t exp(d_d t) phi((d_c - d_d) t),  phi(z) = expm1(z) / z
//     X_n[c][d] = l_n[c] Phi_cd(t'_n) r_n[d],        W = sum_n X_n
//     G = diag(d) - Ainv diag(Q_ii) A
//     times[s]        = (1 / sf) sum_cd Ainv[c][s] W[c][d] A[s][d]
//     jumps[i][j]     = Q_ij sum_cd Ainv[c][i] W[c][d] A[j][d]       (i != j; the diagonal exactly 0)
//     branch_jumps[n] = sum_cd G[c][d] X_n[c][d]                     (a root and a branch with t' = 0: exactly 0)
// The sums have mixed signs; an entry that rounding leaves below zero is returned as 0.0.
//
// heig_basis_kernel: the three changes of basis r = Ainv V, m = A (E o r), l = A^T O for tiles of 16 branches -- from 16 states
// on on the FP64 matrix cores (v_mfma_f64_16x16x4_f64, operands laid out as in history_jump_kernel: the model's matrix is the A
// operand, the tile's vectors the B operand), below that on the vector units.  The matrices are read from global memory: they
// are per column, 512 KB at most, and stay in L2; the tile's vectors go through one LDS buffer of 16 (k + 1) doubles.
// It leaves E_n, r_n and l_n in the call's scratch: 3 ks doubles per branch and column, written once and read once per pair
// tile, against the 2 k doubles per branch (v_n, q_p) the pass streams in -- the price of forming E_n, the division and the
// three products once per branch and not once per tile of pairs.
// heig_pair_kernel: lanes own pairs (c, d): lane = d within a band of 64, CR values of c in registers; the four wavefronts of a
// workgroup take the ids of a piece round robin, each with its own accumulators (no barrier inside the walk, and a branch's
// sum over the pairs for branch_jumps stays inside one wavefront), and are added in wavefront order at the end.  Beyond one tile
// (k > 32: bands of 32 values of c up to 64 states, of 64 beyond) the pairs are tiled over the grid.  The partials are summed in piece order (heig_reduce_kernel), and times / jumps
// come from W by two small products per column in a fixed order (heig_t1_kernel, heig_times_kernel, heig_jumps_kernel).
//
// Phi and the switch on |z|, z = (d_c - d_d) t.  The difference form (E[c] - E[d]) / (d_c - d_d) = E[lo] (e^|z| - 1) / (|d_c - d_d|)
// subtracts two numbers whose ratio is e^|z|: it keeps all but log2(1 / (1 - e^-|z|)) bits -- 1.3 bits at |z| = 0.5, ten
// digits lost at 1e-10, none kept at 0.  The phi form t E[lo] phi(|z|), lo the end with the smaller eigenvalue so that the
// argument is >= 0, is a sum of positive terms 1 + |z| / 2! + |z|^2 / 3! + ... and keeps every digit; below 0.5 the term of
// |z|^15 is under 2e-18 of the first.  So PML_HEIG_SWITCH = 0.5 with 15 terms: either form is good to a few ulp where it is
// used, and no pair costs a transcendental (E_n is k exponentials per branch, formed in heig_basis_kernel).
//
// Bits.  No floating-point atomics.  The nodes are walked in the CALLER's numbering; the pair sum cuts them into pieces of
// PML_HEIG_PIECE ids whatever k is; a wavefront's ids, the order of its additions and the order in which wavefronts and pieces are
// combined are fixed.  Nothing depends on the grid, on the other columns, on the column's position or on which outputs are
// asked for (W is formed in full either way).  The posteriors this reads are the eigen sweeps': their bits follow the schedule.
#pragma once
#include "pml_kernels_history.h"   // (HistSeries, pml_v4f64)

#define PML_HEIG_PIECE 512
#define PML_HEIG_SWITCH 0.5
#define PML_HEIG_TERMS 15

struct PmlHeigArgs {
    const int* parent;              // the library's numbering, as all per-node arrays below
    const int* n_children;
    const int* new_of_old;          // caller's id -> library's id; null = the same
    const double* dist;             // [N]
    const u64* masks;               // [C][N][W]
    const double* bu;               // [C][N][ks]   (tips: not stored, their masks as 0/1)
    const double* post;             // [C][N][ks]
    const double *ev, *A, *Ainv;    // [C][k], [C][k][k], [C][k][k]
    const double *sf, *tau, *tauf;  // [C]
    int N, k, ks, W;
    int col0;                       // first column of the call; the grid's column index counts from it
    int n_pieces;
    int tc, td;                     // tiles of the pairs: tc bands of CR values of c, td bands of 64 values of d
    double* stage;                  // [cols][N][3][ks], CALLER's numbering: E_n, r_n, l_n (l_n = 0: the branch adds nothing)
    double* tprime;                 // [cols][N], caller's numbering: t'_n (0 for a root)
    double* partial;                // [cols][n_pieces][k][k]
    double* Wsum;                   // [cols][k][k]
    double* T1;                     // [cols][k][k]: T1[s][d] = sum_c Ainv[c][s] W[c][d]
    double* qdiag;                  // [cols][k]: Q_ii; null without branch_jumps
    double* G;                      // [cols][k][k]; null without branch_jumps
    double* bpart;                  // [cols][tc td][N]: a tile's share of branch_jumps; null without
    double* times_out;              // [cols][k]
    double* branch_out;             // [cols][N] caller's numbering, or null
    double* jumps_out;              // [cols][k][k], or null
};

// phi(z) = expm1(z) / z for 0 <= z < PML_HEIG_SWITCH: 1 + z / 2! + ... + z^15 / 16!, every term positive
__device__ __forceinline__ double heig_phi(double z) {
    constexpr HistSeries T = hist_series_table();   // inv[m] = 1 / (m + 1)!
    double s = T.inv[PML_HEIG_TERMS];
#pragma unroll
    for (int m = PML_HEIG_TERMS - 1; m >= 1; --m) s = fma(s, z, T.inv[m]);
    return fma(s, z, 1.0);
}

// Phi_cd(t) from the exponentials and eigenvalues of its two ends
__device__ __forceinline__ double heig_Phi(double t, double dc, double dd, double Ec, double Ed) {
    const double diff = dc - dd, z = diff * t, az = fabs(z);
    if (az < PML_HEIG_SWITCH) return t * (z >= 0.0 ? Ed : Ec) * heig_phi(az);
    return (Ec - Ed) / diff;   // (never 0 / 0: equal eigenvalues take the series)
}

// What a thread of a tile of 16 vectors owns, and the product of the model's matrix with the tile (heig_basis_kernel below has the
// layout).  heig_owned: state s and vector b of the idx-th value of this thread; false beyond the tiles.
template <bool MFMA>
__device__ __forceinline__ bool heig_owned(int idx, int kp, int& s, int& b) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (MFMA) {
        const int ta = wave + 4 * (idx >> 2);
        s = 16 * ta + (lane >> 4) + 4 * (idx & 3);
        b = lane & 15;
        return 16 * ta < kp;
    }
    s = threadIdx.x >> 4;
    b = threadIdx.x & 15;
    return true;
}
// res = M X (TR: M^T X) for the values this thread owns; X[b][s] in LDS with the row stride kp + 1
template <bool MFMA>
__device__ __forceinline__ void heig_product(const double* M, bool TR, const double* X, int k, double* res) {
    const int kp = (k + 15) & ~15, LD = kp + 1;
    if (MFMA) {
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lo = lane & 15, hi = lane >> 4;
        const int T = kp >> 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ta = wave + 4 * q;
            pml_v4f64 acc = pml_v4f64{0.0, 0.0, 0.0, 0.0};
            if (ta < T) {   // (uniform over the wavefront)
                const int row = 16 * ta + lo, rc = min(row, k - 1);
                for (int s4 = 0; s4 < kp; s4 += 4) {
                    const int c = s4 + hi, cc = min(c, k - 1);
                    const double m = TR ? M[(size_t)cc * k + rc] : M[(size_t)rc * k + cc];
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64((row < k && c < k) ? m : 0.0, X[lo * LD + c], acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) res[4 * q + reg] = acc[reg];
        }
    } else {
        const int s = min((int)(threadIdx.x >> 4), k - 1), b = threadIdx.x & 15;
        double sum = 0.0;
        for (int c = 0; c < k; ++c) sum = fma(TR ? M[(size_t)c * k + s] : M[(size_t)s * k + c], X[b * LD + c], sum);
        res[0] = sum;
    }
}

// The changes of basis of 16 branches.  grid (ceil(N / 16), column), 256 threads, dynamic LDS: 16 (kp + 1) + 16 doubles, kp = k
// rounded up to 16.  X[b][s], row stride kp + 1 (odd: the 16 branches of an MFMA operand fall into different banks).
// MFMA: a wavefront owns the row tiles ta = wave, wave + 4, ... of the result (at most four up to 256 states); per step of four
// states the A operand is M[16 ta + lo][4 s + hi] (TR: M[4 s + hi][16 ta + lo]), the B operand X[lo][4 s + hi]; D: branch = lane
// & 15, state = 16 ta + (lane >> 4) + 4 reg.  Otherwise (k < 16) thread t owns state t >> 4 of branch t & 15.
template <bool MFMA>
__global__ void __launch_bounds__(256) heig_basis_kernel(PmlHeigArgs A) {
    extern __shared__ double heig_lds[];
    constexpr int NR = MFMA ? 16 : 1;
    const int k = A.k, ks = A.ks, kp = (k + 15) & ~15, LD = kp + 1;
    double* X = heig_lds;
    double* tb = heig_lds + 16 * LD;   // t' of the tile's branches; < 0: not a branch (a root, beyond N)
    const int col = A.col0 + blockIdx.y;
    const size_t colN = (size_t)col * A.N;
    const double* ev = A.ev + (size_t)col * k;
    const double* Am = A.A + (size_t)col * k * k;
    const double* Ai = A.Ainv + (size_t)col * k * k;
    const int i0 = blockIdx.x * 16;
    auto owned = [&](int idx, int& s, int& b) -> bool { return heig_owned<MFMA>(idx, kp, s, b); };
    auto product = [&](const double* M, bool TR, double* res) { heig_product<MFMA>(M, TR, X, k, res); };

    // X = V; t' of the branches
    for (int e = threadIdx.x; e < 16 * kp; e += 256) {
        const int b = e / kp, s = e % kp;
        const int i = min(i0 + b, A.N - 1);
        const int n = A.new_of_old ? A.new_of_old[i] : i;
        const size_t row = colN + n;
        const int ss = min(s, k - 1);
        const u64 m = A.masks[row * A.W + (ss >> 6)];
        const double x = A.bu[row * ks + ss];
        const bool tip = A.n_children[n] == 0;
        const bool allowed = s < k && ((m >> (ss & 63)) & 1ull);
        X[b * LD + s] = allowed ? (tip ? 1.0 : x) : 0.0;
    }
    if (threadIdx.x < 16) {
        const int i = min(i0 + (int)threadIdx.x, A.N - 1);
        const int n = A.new_of_old ? A.new_of_old[i] : i;
        const bool branch = i0 + (int)threadIdx.x < A.N && A.parent[n] >= 0;
        const double t = (A.dist[n] + A.tau[col]) * (A.tauf[col] * A.sf[col]);
        tb[threadIdx.x] = branch ? t : -1.0;
        if (i0 + (int)threadIdx.x < A.N) A.tprime[(size_t)blockIdx.y * A.N + i] = branch ? t : 0.0;
    }
    __syncthreads();

    double res[NR];
    // r = Ainv V; E; X <- E o r
    product(Ai, false, res);
    __syncthreads();
#pragma unroll
    for (int idx = 0; idx < NR; ++idx) {
        int s, b;
        if (!owned(idx, s, b)) continue;
        const double t = tb[b];
        const bool live = s < k && i0 + b < A.N;
        const double E = exp(ev[min(s, k - 1)] * fmax(t, 0.0));
        if (live) {
            double* st = A.stage + ((size_t)blockIdx.y * A.N + (i0 + b)) * 3 * ks;
            st[s] = E;
            st[ks + s] = res[idx];
        }
        if (s < kp) X[b * LD + s] = s < k ? E * res[idx] : 0.0;
    }
    __syncthreads();
    // m = A (E o r); X <- o = q_p / m
    product(Am, false, res);
    __syncthreads();
#pragma unroll
    for (int idx = 0; idx < NR; ++idx) {
        int s, b;
        if (!owned(idx, s, b)) continue;
        const int i = min(i0 + b, A.N - 1);
        const int n = A.new_of_old ? A.new_of_old[i] : i;
        const int pp = max(A.parent[n], 0);
        const double q = A.post[(colN + pp) * ks + min(s, k - 1)];
        const double m = res[idx];
        const bool on = s < k && tb[b] > 0.0 && q > 0.0 && m > 0.0;
        if (s < kp) X[b * LD + s] = on ? q / m : 0.0;
    }
    __syncthreads();
    // l = A^T o
    product(Am, true, res);
#pragma unroll
    for (int idx = 0; idx < NR; ++idx) {
        int s, b;
        if (!owned(idx, s, b)) continue;
        if (s < k && i0 + b < A.N) A.stage[((size_t)blockIdx.y * A.N + (i0 + b)) * 3 * ks + 2 * ks + s] = tb[b] > 0.0 ? res[idx] : 0.0;
    }
}

// Q_ii.  grid (column), thread i
static __global__ void __launch_bounds__(256) heig_qdiag_kernel(PmlHeigArgs A) {
    const int k = A.k, i = threadIdx.x;
    if (i >= k) return;
    const size_t col = A.col0 + blockIdx.x;
    const double *ev = A.ev + col * k, *Am = A.A + col * k * k, *Ai = A.Ainv + col * k * k;
    double q = 0.0;
    for (int m = 0; m < k; ++m) q = fma(Am[(size_t)i * k + m] * ev[m], Ai[(size_t)m * k + i], q);
    A.qdiag[(size_t)blockIdx.x * k + i] = q;
}

// G = diag(d) - Ainv diag(Q_ii) A.  grid (k k / 256, column)
static __global__ void __launch_bounds__(256) heig_g_kernel(PmlHeigArgs A) {
    const int k = A.k;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= k * k) return;
    const int c = idx / k, d = idx % k;
    const size_t col = A.col0 + blockIdx.y;
    const double *Am = A.A + col * k * k, *Ai = A.Ainv + col * k * k, *qd = A.qdiag + (size_t)blockIdx.y * k;
    double s = 0.0;
    for (int i = 0; i < k; ++i) s = fma(Ai[(size_t)c * k + i] * qd[i], Am[(size_t)i * k + d], s);
    A.G[(size_t)blockIdx.y * k * k + idx] = (c == d ? A.ev[col * k + c] : 0.0) - s;
}

// The pair sum of one piece and one tile of pairs.  grid (piece, tile, column); tile = band of c (CR values) x band of d (64).
template <int CR>
__global__ void __launch_bounds__(256) heig_pair_kernel(PmlHeigArgs A) {
    __shared__ double buf[CR * 64];   // G's tile in the walk, the wavefronts' sums afterwards
    const int k = A.k, ks = A.ks;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int tile = blockIdx.y, c0 = (tile / A.td) * CR, d = (tile % A.td) * 64 + lane;
    const bool d_in = d < k;
    const int dcl = min(d, k - 1);
    const int col = A.col0 + blockIdx.z;
    const double* ev = A.ev + (size_t)col * k;
    const double ev_d = ev[dcl];
    const bool with_branch = A.bpart != nullptr;
    if (with_branch) {
        const double* G = A.G + (size_t)blockIdx.z * k * k;
        for (int e = threadIdx.x; e < CR * 64; e += 256) {
            const int c = c0 + (e >> 6), dd = (tile % A.td) * 64 + (e & 63);
            buf[e] = (c < k && dd < k) ? G[(size_t)min(c, k - 1) * k + min(dd, k - 1)] : 0.0;
        }
        __syncthreads();
    }
    double acc[CR];
#pragma unroll
    for (int j = 0; j < CR; ++j) acc[j] = 0.0;
    const int i0 = blockIdx.x * PML_HEIG_PIECE, i1 = min(A.N, i0 + PML_HEIG_PIECE);
    for (int i = i0 + wave; i < i1; i += 4) {
        const double* st = A.stage + ((size_t)blockIdx.z * A.N + i) * 3 * ks;
        const double t = A.tprime[(size_t)blockIdx.z * A.N + i];
        const double E_d = st[dcl];
        const double r_d = d_in ? st[ks + dcl] : 0.0;
        double bj = 0.0;
#pragma unroll
        for (int j = 0; j < CR; ++j) {
            const int c = c0 + j, cc = min(c, k - 1);   // (uniform over the wavefront)
            const double l_c = c < k ? st[2 * ks + cc] : 0.0;
            const double x = l_c * heig_Phi(t, ev[cc], ev_d, st[cc], E_d) * r_d;
            acc[j] += x;
            if (with_branch) bj = fma(buf[j * 64 + lane], x, bj);
        }
        if (with_branch) {
            bj = group_sum<64>(bj);
            if (lane == 0) A.bpart[((size_t)blockIdx.z * gridDim.y + tile) * A.N + i] = bj;
        }
    }
    // the wavefronts' sums in wavefront order
    __syncthreads();
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int j = 0; j < CR; ++j) buf[j * 64 + lane] = w == 0 ? acc[j] : buf[j * 64 + lane] + acc[j];
        }
        __syncthreads();
    }
    double* out = A.partial + ((size_t)blockIdx.z * A.n_pieces + blockIdx.x) * k * k;
    for (int e = threadIdx.x; e < CR * 64; e += 256) {
        const int c = c0 + (e >> 6), dd = (tile % A.td) * 64 + (e & 63);
        if (c < k && dd < k) out[(size_t)c * k + dd] = buf[e];
    }
}

// W: the pieces' partials in piece order.  grid (k k / 256, column)
static __global__ void __launch_bounds__(256) heig_reduce_kernel(PmlHeigArgs A) {
    const int k = A.k;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= k * k) return;
    const double* part = A.partial + (size_t)blockIdx.y * A.n_pieces * k * k + idx;
    double s = 0.0;
    for (int j = 0; j < A.n_pieces; ++j) s += part[(size_t)j * k * k];
    A.Wsum[(size_t)blockIdx.y * k * k + idx] = s;
}

// T1[s][d] = sum_c Ainv[c][s] W[c][d], c ascending.  grid (k k / 256, column)
static __global__ void __launch_bounds__(256) heig_t1_kernel(PmlHeigArgs A) {
    const int k = A.k;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= k * k) return;
    const int s = idx / k, d = idx % k;
    const double* Ai = A.Ainv + (size_t)(A.col0 + blockIdx.y) * k * k;
    const double* W = A.Wsum + (size_t)blockIdx.y * k * k;
    double sum = 0.0;
    for (int c = 0; c < k; ++c) sum = fma(Ai[(size_t)c * k + s], W[(size_t)c * k + d], sum);
    A.T1[(size_t)blockIdx.y * k * k + idx] = sum;
}

// times[s] = (1 / sf) sum_d T1[s][d] A[s][d], d ascending.  grid (column), thread s
static __global__ void __launch_bounds__(256) heig_times_kernel(PmlHeigArgs A) {
    const int k = A.k, s = threadIdx.x;
    if (s >= k) return;
    const size_t col = A.col0 + blockIdx.x;
    const double* Am = A.A + col * k * k + (size_t)s * k;
    const double* T1 = A.T1 + (size_t)blockIdx.x * k * k + (size_t)s * k;
    double sum = 0.0;
    for (int d = 0; d < k; ++d) sum = fma(T1[d], Am[d], sum);
    sum /= A.sf[col];
    A.times_out[(size_t)blockIdx.x * k + s] = sum > 0.0 ? sum : 0.0;
}

// jumps[i][j] = Q_ij sum_d T1[i][d] A[j][d], Q_ij = sum_m A[i][m] d_m Ainv[m][j]; the diagonal 0.  grid (k k / 256, column)
static __global__ void __launch_bounds__(256) heig_jumps_kernel(PmlHeigArgs A) {
    const int k = A.k;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= k * k) return;
    const int i = idx / k, j = idx % k;
    const size_t col = A.col0 + blockIdx.y;
    const double *ev = A.ev + col * k, *Am = A.A + col * k * k, *Ai = A.Ainv + col * k * k;
    const double* T1 = A.T1 + (size_t)blockIdx.y * k * k + (size_t)i * k;
    double sum = 0.0, q = 0.0;
    for (int d = 0; d < k; ++d) sum = fma(T1[d], Am[(size_t)j * k + d], sum);
    for (int m = 0; m < k; ++m) q = fma(Am[(size_t)i * k + m] * ev[m], Ai[(size_t)m * k + j], q);
    const double v = q * sum;
    A.jumps_out[(size_t)blockIdx.y * k * k + idx] = (i != j && v > 0.0) ? v : 0.0;
}

// branch_jumps[i] = the tiles' shares in tile order.  grid (N / 256, column)
static __global__ void __launch_bounds__(256) heig_branch_kernel(PmlHeigArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.N) return;
    const int tiles = A.tc * A.td;
    const double* part = A.bpart + (size_t)blockIdx.y * tiles * A.N + i;
    double s = 0.0;
    for (int t = 0; t < tiles; ++t) s += part[(size_t)t * A.N];
    A.branch_out[(size_t)blockIdx.y * A.N + i] = s > 0.0 ? s : 0.0;
}
