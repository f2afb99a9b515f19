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
// What the sums per time interval (pml_kernels_history_time_eigen.h) share with these -- the arguments, Phi, heig_basis_kernel and
// its products, the tiles and the epilogue of the pair sum, the transforms of W -- is pml_kernels_history_eigen_shared.h's.
// heig_basis_kernel: the three changes of basis r = Ainv V, m = A (E o r), l = A^T O for tiles of 16 branches -- from 16 states
// on on the FP64 matrix cores (v_mfma_f64_16x16x4_f64, operands laid out as in hist_jump_product: the model's matrix is the A
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
#include "pml_kernels_history_eigen_shared.h"

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

// The pair sum of one piece of ids and one tile of pairs (heig_tile), with a branch's sum over the tile's pairs for
// branch_jumps, which stays inside one wavefront.  grid (piece, tile, column)
template <int CR>
__global__ void __launch_bounds__(256) heig_pair_kernel(PmlHeigArgs A) {
    __shared__ double buf[CR * 64];   // G's tile in the walk, the wavefronts' sums afterwards
    const int k = A.k, ks = A.ks;
    const HeigTile t = heig_tile<CR>(A);
    const bool with_branch = A.bpart != nullptr;
    if (with_branch) {
        const double* G = A.G + (size_t)blockIdx.z * k * k;
        for (int e = threadIdx.x; e < CR * 64; e += 256) {
            const int c = t.c0 + (e >> 6), dd = t.d0 + (e & 63);
            buf[e] = (c < k && dd < k) ? G[(size_t)min(c, k - 1) * k + min(dd, k - 1)] : 0.0;
        }
        __syncthreads();
    }
    double acc[CR];
#pragma unroll
    for (int j = 0; j < CR; ++j) acc[j] = 0.0;
    const int i0 = blockIdx.x * PML_HEIG_PIECE, i1 = min(A.N, i0 + PML_HEIG_PIECE);
    for (int i = i0 + t.wave; i < i1; i += 4) {
        const double* st = A.stage + ((size_t)blockIdx.z * A.N + i) * 3 * ks;
        const double tp = A.tprime[(size_t)blockIdx.z * A.N + i];
        const double E_d = st[t.dcl];
        const double r_d = t.d_in ? st[ks + t.dcl] : 0.0;
        double bj = 0.0;
#pragma unroll
        for (int j = 0; j < CR; ++j) {
            const int c = t.c0 + j, cc = min(c, k - 1);   // (uniform over the wavefront)
            const double l_c = c < k ? st[2 * ks + cc] : 0.0;
            const double x = l_c * heig_Phi(tp, t.ev[cc], t.ev_d, st[cc], E_d) * r_d;
            acc[j] += x;
            if (with_branch) bj = fma(buf[j * 64 + t.lane], x, bj);
        }
        if (with_branch) {
            bj = group_sum<64>(bj);
            if (t.lane == 0) A.bpart[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * A.N + i] = bj;
        }
    }
    __syncthreads();   // (G's tile has been read)
    heig_tile_sums<CR>(t, buf, acc, k, A.partial + ((size_t)blockIdx.z * A.n_pieces + blockIdx.x) * k * k);
}

// W: the pieces' partials in piece order.  grid (k k / 256, column), as the two kernels after it
static __global__ void __launch_bounds__(256) heig_reduce_kernel(PmlHeigArgs A) {
    const int k = A.k, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= k * k) return;
    A.Wsum[(size_t)blockIdx.y * k * k + idx] = pml_piece_sum(A.partial + (size_t)blockIdx.y * A.n_pieces * k * k + idx, (size_t)k * k, 0, A.n_pieces);
}

static __global__ void __launch_bounds__(256) heig_t1_kernel(PmlHeigArgs A) {
    const int k = A.k, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < k * k) heig_t1(A, blockIdx.y, idx, A.Wsum + (size_t)blockIdx.y * k * k, A.T1 + (size_t)blockIdx.y * k * k);
}

static __global__ void __launch_bounds__(256) heig_jumps_kernel(PmlHeigArgs A) {
    const int k = A.k, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < k * k) heig_jumps(A, blockIdx.y, idx, A.T1 + (size_t)blockIdx.y * k * k, A.jumps_out + (size_t)blockIdx.y * k * k);
}

// grid (column), thread s
static __global__ void __launch_bounds__(256) heig_times_kernel(PmlHeigArgs A) {
    const int k = A.k;
    if ((int)threadIdx.x < k) heig_times(A, blockIdx.x, threadIdx.x, A.T1 + (size_t)blockIdx.x * k * k, A.times_out + (size_t)blockIdx.x * k);
}

// branch_jumps[i] = the tiles' shares in tile order.  grid (N / 256, column)
static __global__ void __launch_bounds__(256) heig_branch_kernel(PmlHeigArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.N) return;
    const int tiles = A.tc * A.td;
    const double s = pml_piece_sum(A.bpart + (size_t)blockIdx.y * tiles * A.N + i, A.N, 0, tiles);
    A.branch_out[(size_t)blockIdx.y * A.N + i] = s > 0.0 ? s : 0.0;
}
