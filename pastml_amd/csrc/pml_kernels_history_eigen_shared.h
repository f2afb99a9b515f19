// What the exact histories of the eigen-decomposed models share: the whole-tree sums (pml_kernels_history_eigen.h) and the sums
// per time interval (pml_kernels_history_time_eigen.h) both stage E_n, r_n, l_n per branch (heig_basis_kernel, which both entries
// launch through launch_heig_basis), sum l[c] Phi_cd r[d] over tiles of pairs with the same tile coordinates and the same
// wavefront-order epilogue, and turn W into times and jumps by the same two small products; the argument struct, Phi and the
// products of a tile of 16 vectors with the model's matrix are here as well.  Apart from heig_basis_kernel, a template, no kernel
// lives here: a unit that includes this emits what it launches and nothing else.
#pragma once
#include "pml_kernels_history_shared.h"   // (HistSeries, pml_v4f64, pml_piece_sum)

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

// ---- the pair sum: a tile of pairs is a band of CR values of c x a band of 64 values of d.  grid (piece, tile, column); lanes
// own pairs: lane = d within the band, CR values of c in registers; the four wavefronts of a workgroup take the items of a
// piece round robin, each with its own accumulators (no barrier inside the walk), and are added in wavefront order at the end.
struct HeigTile {
    int wave, lane;
    int c0, d0;          // the tile's first c and d
    int dcl;             // this lane's d, clamped to a state
    bool d_in;           // this lane's d is a state
    const double* ev;    // the column's eigenvalues
    double ev_d;
};
template <int CR>
__device__ __forceinline__ HeigTile heig_tile(const PmlHeigArgs& A) {
    HeigTile t;
    t.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), t.lane = threadIdx.x & 63;
    t.c0 = (blockIdx.y / A.td) * CR, t.d0 = (blockIdx.y % A.td) * 64;
    t.d_in = t.d0 + t.lane < A.k;
    t.dcl = min(t.d0 + t.lane, A.k - 1);
    t.ev = A.ev + (size_t)(A.col0 + blockIdx.z) * A.k;
    t.ev_d = t.ev[t.dcl];
    return t;
}
// The wavefronts' sums in wavefront order through buf [CR][64] (free when the first wavefront comes here), and the tile's
// entries of the piece's partial out [k][k]
template <int CR>
__device__ __forceinline__ void heig_tile_sums(const HeigTile& t, double* buf, const double (&acc)[CR], int k, double* out) {
    for (int w = 0; w < 4; ++w) {
        if (t.wave == w) {
#pragma unroll
            for (int j = 0; j < CR; ++j) buf[j * 64 + t.lane] = w == 0 ? acc[j] : buf[j * 64 + t.lane] + acc[j];
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < CR * 64; e += 256) {
        const int c = t.c0 + (e >> 6), dd = t.d0 + (e & 63);
        if (c < k && dd < k) out[(size_t)c * k + dd] = buf[e];
    }
}

// ---- from one W (the whole tree's, or a bin's: pml_piece_sum over its pieces) to times and jumps, by two small products in a
// fixed order.  column: the grid's; W, T1: the k k doubles of this W; the outputs: the k (k k) entries that belong to it.
// T1[s][d] = sum_c Ainv[c][s] W[c][d], c ascending; idx = s k + d
__device__ __forceinline__ void heig_t1(const PmlHeigArgs& A, int column, int idx, const double* W, double* T1) {
    const int k = A.k, s = idx / k, d = idx % k;
    const double* Ai = A.Ainv + (size_t)(A.col0 + column) * k * k;
    double sum = 0.0;
    for (int c = 0; c < k; ++c) sum = fma(Ai[(size_t)c * k + s], W[(size_t)c * k + d], sum);
    T1[idx] = sum;
}
// times[s] = (1 / sf) sum_d T1[s][d] A[s][d], d ascending
__device__ __forceinline__ void heig_times(const PmlHeigArgs& A, int column, int s, const double* T1, double* times) {
    const int k = A.k;
    const size_t col = A.col0 + column;
    const double* Am = A.A + col * k * k + (size_t)s * k;
    T1 += (size_t)s * k;
    double sum = 0.0;
    for (int d = 0; d < k; ++d) sum = fma(T1[d], Am[d], sum);
    sum /= A.sf[col];
    times[s] = sum > 0.0 ? sum : 0.0;
}
// jumps[i][j] = Q_ij sum_d T1[i][d] A[j][d], Q_ij = sum_m A[i][m] d_m Ainv[m][j]; the diagonal 0; idx = i k + j
__device__ __forceinline__ void heig_jumps(const PmlHeigArgs& A, int column, int idx, const double* T1, double* jumps) {
    const int k = A.k, i = idx / k, j = idx % k;
    const size_t col = A.col0 + column;
    const double *ev = A.ev + col * k, *Am = A.A + col * k * k, *Ai = A.Ainv + col * k * k;
    T1 += (size_t)i * k;
    double sum = 0.0, q = 0.0;
    for (int d = 0; d < k; ++d) sum = fma(T1[d], Am[(size_t)j * k + d], sum);
    for (int m = 0; m < k; ++m) q = fma(Am[(size_t)i * k + m] * ev[m], Ai[(size_t)m * k + j], q);
    const double v = q * sum;
    jumps[idx] = (i != j && v > 0.0) ? v : 0.0;
}
