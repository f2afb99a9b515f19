// Exact expected transition counts: the n_repetitions -> infinity limit of marginal_counts (pastml/ml.py:753-862), all columns
// of a batch in one pass (pml_expected_counts).
//
// The quantity, per column and tree, nodes in level order, in units "per scenario".  M_n[a][b] is the reference's conditional
// (ml.py:819-824):  w_n[b] = BU_n[b] pi_b mask_n[b],  M_n[a][b] = w_n[b] P_n[b][a] / sum_b' w_n[b'] P_n[b'][a];  rows a with
// q_parent[a] == 0 are never used (ml.py:831).  Masks are the ones the marginal pass ran with.
//   * q_root = marginal posterior of the root (ml.py:794-798); q_n = q_parent . M_n for every other node.  The models are
//     reversible and M_n is the posterior conditional of n given its parent, so q_n IS the marginal posterior of n: the kernels
//     read the posterior table instead of propagating.
//   * pair (p, n) with neither end altered by the zero-branch handling:  result[a][b] += q_p[a] M_n[a][b],
//     same_p[a] += q_p[a] M_n[a][a].
//   * pair with an altered end (ml.py:806-812, 840-855): ps = to_initial(q_p, p) if p is altered else q_p; ci likewise for n;
//     norm = ci / sum(ci); for every i with ps[i] > 0: result[i][:] += norm ps[i], same_p[i] += norm[i] ps[i];
//     to_initial(q, x) = q * initial_mask_x renormalised to sum 1, or initial_mask_x / its sum if that product is all zero.
//     These pairs are the caller's (pastml_amd.ml.expected_counts): the kernels leave them out when `altered` is given.
//   * after the children of p (ml.py:859-860):  result[i][i] -= min(ps[i], same_p[i]).
//
// F81 family (P[b][a] = (1 - e) pi_a + e [a == b]):  with S_n = sum_b w_n[b] and den_n[a] = (1 - e) pi_a S_n + e w_n[a] the
// unaltered part is  sum_n u_n (x) w_n + diag(sum_n q_p[a] e w_n[a] / den_n[a]),  u_n[a] = q_p[a] (1 - e) pi_a / den_n[a]:
// U^T W on the FP64 matrix cores (expected_f81_kernel), the diagonal terms in the pass over the parents.
// Matrix models (HKY, eigen): the per-branch term is the elementwise product of P_n^T, w_n and q_p / den_n, read from the
// materialised P(t), or from its window (expected_matrix_kernel) -- k^2 doubles per branch, memory-bound.
//
// Bits.  No floating-point atomics.  The nodes are walked in the CALLER's numbering and cut into pieces of a fixed number of
// ids (a function of k and the model kind only); a workgroup owns one piece's partial k x k (or one piece of parents' partial
// diagonal), and expected_reduce_kernel sums the partials in piece order.  Nothing depends on the grid, on the schedule of the
// sweeps, on the library's own numbering or on the column.
#pragma once
#include "pml_kernels_pij.h"

struct PmlExpArgs {
    const int* parent;              // the library's numbering, as all per-node arrays below
    const int* first_child;
    const int* n_children;
    const int* new_of_old;          // caller's id -> library's id; null = the same
    const unsigned char* altered;   // [N] (library's numbering) or null
    const u64* masks;               // [C][N][W]
    const double* pi;               // [C][ks]
    const double* bu;               // [C][N][ks]   (tips: not stored, their masks as 0/1)
    const double* post;             // [C][N][ks]
    const double* E;                // [C][N]       F81 family
    const double* P;                // [C][N][k][ks] matrix models: P^T per branch
    int N, k, ks, W;
    int col0;                       // first column of the call; blockIdx.z counts from it
    int piece, n_pieces;            // ids per piece of the branch pass
    int ppiece, n_ppieces;          // ids per piece of the pass over the parents
    double* partial;                // [cols][n_pieces][k][k]
    double* corr;                   // [cols][n_ppieces][k]   diagonal terms of the parents
    double* rowsum;                 // [cols][N]  F81: S_n (library's numbering), written by the branch pass
    double* dterm;                  // [cols][N][k] matrix models: q_p[a] M_n[a][a] per branch, written by the branch pass
    double* same;                   // [cols][N][k] caller's numbering, or null: same_p of the parents of a pair with an altered end
    double* out;                    // [cols][k][k]
    // P(t) in a window (pml_pij_window.h; expected_matrix_kernel<CK, true>): this launch is the run of the pieces piece0 ..
    // piece0 + gridDim.x, P is the window [cols of the call][win_B][k][ks] and the branch of id i lies in slot i - piece0 piece
    int piece0;
    long long win_B;
};

// w_n[b] = BU_n[b] pi_b mask_n[b]; row = col * N + n.  Every load is issued whatever the mask, the tip flag or b say (a clamped
// address, a select afterwards): the loads of a step are independent and overlap instead of forming a chain mask -> vector.
__device__ __forceinline__ double exp_weight(const PmlExpArgs& A, int col, size_t row, bool tip, int b) {
    const int bb = min(b, A.k - 1);
    const u64 m = A.masks[row * A.W + (bb >> 6)];
    const double v = A.bu[row * A.ks + bb];
    const double p = A.pi[(size_t)col * A.ks + bb];
    const bool allowed = b < A.k && ((m >> (bb & 63)) & 1ull);
    return allowed ? (tip ? p : v * p) : 0.0;
}

// S_n = sum_b w_n[b] of every node with a parent, for more than 64 states (below, the branch pass forms it from the tiles it holds).
// grid (nodes / 16, column); 16 lanes per node, the states in tiles of 16, the lanes' sums by DPP: the order is fixed.
static __global__ void __launch_bounds__(256) expected_rowsum_kernel(PmlExpArgs A) {
    const int lo = threadIdx.x & 15;
    const int id = blockIdx.x * 16 + (int)(threadIdx.x >> 4);
    const int n = min(id, A.N - 1);   // (the lanes beyond the last node read it again and store nothing)
    const int col = A.col0 + blockIdx.y;
    const size_t row = (size_t)col * A.N + n;
    const bool tip = A.n_children[n] == 0;
    const int T = (A.k + 15) >> 4;
    double S = 0.0;
    for (int tt = 0; tt < T; ++tt) S += exp_weight(A, col, row, tip, 16 * tt + lo);
    S = group_sum<16>(S);
    if (lo == 0 && id < A.N) A.rowsum[(size_t)blockIdx.y * A.N + n] = S;
}

// F81 family, any k <= 512.  grid (piece, tile group, column); a wavefront owns the 16 rows a of one band and four bands of
// columns b; per step the four lane rows (hi) hold four consecutive branches: A[m][kk] = u_kk[a0 + m], B[kk][n] = w_kk[b0 + n]
// (v_mfma_f64_16x16x4_f64; D: col = lane & 15, row = (lane >> 4) + 4 reg).  States beyond k and ids that are roots, beyond the
// piece or ends of an altered pair enter as zeros.
// WIDE = 0: up to 64 states, one tile group, and the loop over the steps is unrolled by four so that the loads of 16 branches are in
// flight together (a step is a chain id -> parent -> posterior row: alone it waits for HBM twice).
template <int WIDE>
__global__ void __launch_bounds__(256) expected_f81_kernel(PmlExpArgs A) {
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
    const int i0 = blockIdx.x * A.piece, i1 = min(A.N, i0 + A.piece);
    const bool writes_S = blockIdx.y == 0 && wave == 0 && lo == 0;
    const int a_c = min(a, k - 1);
    auto step = [&](int base) {
        // (ids beyond the piece and roots read node 0 / parent 0 and are zeroed by the selects below: no load waits for a test)
        const int i = min(base + hi, i1 - 1);
        const int n = A.new_of_old ? A.new_of_old[i] : i;
        const int p = A.parent[n];
        bool valid = base + hi < i1 && p >= 0;
        const int pp = max(p, 0);
        const bool tip = A.n_children[n] == 0;
        const size_t row = colN + n;
        const double e = A.E[row];
        const double q = A.post[(colN + pp) * ks + a_c];
        const bool alt = A.altered != nullptr && (A.altered[n] | A.altered[pp]);
        double w[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) w[t] = exp_weight(A, col, row, tip, 16 * (4 * gb + t) + lo);
        double S = 0.0, wa = 0.0;
        if (!WIDE) {   // up to 64 states: the four tiles are the whole row
            S = ((w[0] + w[1]) + w[2]) + w[3];
#pragma unroll
            for (int t = 0; t < 4; ++t) wa = t == wave ? w[t] : wa;
            S = group_sum<16>(S);
            if (valid && writes_S) A.rowsum[(size_t)blockIdx.z * A.N + n] = S;
        } else {   // more than 64 states: S_n comes from expected_rowsum_kernel, every block of the result would form it again
            S = A.rowsum[(size_t)blockIdx.z * A.N + n];
            wa = exp_weight(A, col, row, tip, a);
        }
        valid = valid && !alt;
        const double den = (1.0 - e) * pi_a * S + e * wa;
        const double u = (valid && a < k && q > 0.0 && den > 0.0) ? q * (1.0 - e) * pi_a / den : 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(u, valid ? w[t] : 0.0, acc[t], 0, 0, 0);
    };
    if (!WIDE) {
        // (by hand: the lane exchanges and the MFMA are convergent, which keeps the compiler from unrolling a loop with a
        // remainder; steps beyond the piece are all-zero operands)
        for (int base = i0; base < i1; base += 16) {
            step(base);
            step(base + 4);
            step(base + 8);
            step(base + 12);
        }
    } else {
        for (int base = i0; base < i1; base += 4) step(base);
    }
    double* out = A.partial + ((size_t)blockIdx.z * A.n_pieces + blockIdx.x) * k * k;
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

// Matrix models, k <= 64 CK.  grid (piece, row group, column); the four wavefronts of a workgroup share the rows of the group
// round robin (32 / CK rows each), the lanes hold the columns b = lane + 64 c.  Per branch and row a: den = sum_b w[b] Pt[a][b]
// over the wavefront (fixed order), then acc += q_p[a] / den * w[b] Pt[a][b].  The diagonal entry goes to dterm for the pass
// over the parents.
// WIN: the pieces of one run, P(t) from the window (PmlExpArgs::piece0); a piece's partial, its ids and their order are the same.
template <int CK, bool WIN = false>
__global__ void __launch_bounds__(256) expected_matrix_kernel(PmlExpArgs A) {
    constexpr int RW = 32 / CK;
    const int k = A.k, ks = A.ks;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = A.col0 + blockIdx.z;
    const size_t colN = (size_t)col * A.N;
    const int a_base = blockIdx.y * (4 * RW) + wave;
    double acc[RW][CK];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int c = 0; c < CK; ++c) acc[r][c] = 0.0;
    const int piece_x = WIN ? A.piece0 + (int)blockIdx.x : (int)blockIdx.x;
    const int i0 = piece_x * A.piece, i1 = min(A.N, i0 + A.piece);
    for (int i = i0; i < i1; ++i) {
        const int n = A.new_of_old ? A.new_of_old[i] : i;
        const int p = A.parent[n];
        if (p < 0) continue;
        if (A.altered != nullptr && (A.altered[n] | A.altered[p])) continue;
        const bool tip = A.n_children[n] == 0;
        const size_t row = colN + n;
        double w[CK];
#pragma unroll
        for (int c = 0; c < CK; ++c) w[c] = exp_weight(A, col, row, tip, lane + 64 * c);
        const double* Pt;
        if constexpr (WIN) Pt = A.P + ((size_t)blockIdx.z * (size_t)A.win_B + (size_t)(i - A.piece0 * A.piece)) * (size_t)k * ks;
        else Pt = A.P + row * (size_t)k * ks;
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const int a = a_base + 4 * r;
            if (a >= k) continue;   // (uniform over the wavefront)
            double prod[CK], den = 0.0;
#pragma unroll
            for (int c = 0; c < CK; ++c) {
                const int b = lane + 64 * c;
                // (an eigen model's P(0) carries +-1e-17 where the exact value is 0: clamped, as the sweeps and the sampler do)
                prod[c] = b < k ? w[c] * fmax(Pt[(size_t)a * ks + b], 0.0) : 0.0;
                den += prod[c];
            }
            den = group_sum<64>(den);
            const double q = A.post[(colN + p) * ks + a];
            const double f = (q > 0.0 && den > 0.0) ? q / den : 0.0;
#pragma unroll
            for (int c = 0; c < CK; ++c) {
                const double v = f * prod[c];
                acc[r][c] += v;
                if (lane + 64 * c == a) A.dterm[((size_t)blockIdx.z * A.N + n) * k + a] = v;
            }
        }
    }
    double* out = A.partial + ((size_t)blockIdx.z * A.n_pieces + piece_x) * k * k;
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int a = a_base + 4 * r;
        if (a >= k) continue;
#pragma unroll
        for (int c = 0; c < CK; ++c) {
            const int b = lane + 64 * c;
            if (b < k) out[(size_t)a * k + b] = acc[r][c];
        }
    }
}

// The pass over the parents.  grid (piece of ids, column); thread = (slot, state a): KP = the power of two >= k (at most 256)
// threads per slot, a slot walks the ids i0 + slot, i0 + slot + slots, ... of the piece.  Per parent p, over its children in
// child order: same_p[a] = sum q_p[a] M_n[a][a] (F81: formed here from S_n; matrix models: read from dterm), F81 also
// eterm[a] = sum q_p[a] e w_n[a] / den_n[a], the diagonal part of the branch term that the rank-one product does not carry.
// A parent none of whose pairs has an altered end contributes eterm - min(q_p, same_p) to the diagonal; another one eterm only,
// and its same_p goes out for the caller.  The slots' sums are combined in slot order.
static __global__ void __launch_bounds__(256) expected_parents_kernel(PmlExpArgs A) {
    __shared__ double red[256 * 2];
    const int k = A.k, ks = A.ks;
    int KP = 1;
    while (KP < k && KP < 256) KP <<= 1;
    const int slots = 256 / KP, slot = threadIdx.x / KP, a0 = threadIdx.x % KP;
    const int col = A.col0 + blockIdx.y;
    const size_t colN = (size_t)col * A.N;
    const bool f81 = A.P == nullptr;
    const int i0 = blockIdx.x * A.ppiece, i1 = min(A.N, i0 + A.ppiece);
    double total[2] = {0.0, 0.0};
    for (int i = i0 + slot; i < i1; i += slots) {
        const int p = A.new_of_old ? A.new_of_old[i] : i;
        const int nc = A.n_children[p];
        if (nc == 0) continue;
        const int fc = A.first_child[p];
        const bool p_alt = A.altered != nullptr && A.altered[p];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int a = a0 + h * KP;
            if (a >= k) continue;
            const double q = A.post[(colN + p) * ks + a];
            const double pi_a = A.pi[(size_t)col * ks + a];
            double same = 0.0, eterm = 0.0;
            bool dirty = p_alt;
            for (int j = 0; j < nc; ++j) {
                const int n = fc + j;
                if (p_alt || (A.altered != nullptr && A.altered[n])) {
                    dirty = true;
                    continue;
                }
                if (f81) {
                    const size_t row = colN + n;
                    const double e = A.E[row];
                    const double wa = exp_weight(A, col, row, A.n_children[n] == 0, a);
                    const double den = (1.0 - e) * pi_a * A.rowsum[(size_t)blockIdx.y * A.N + n] + e * wa;
                    if (q > 0.0 && den > 0.0) {
                        const double f = q * wa / den;
                        eterm += f * e;
                        same += f * ((1.0 - e) * pi_a + e);
                    }
                } else {
                    same += A.dterm[((size_t)blockIdx.y * A.N + n) * k + a];
                }
            }
            if (dirty) {
                if (A.same != nullptr) A.same[((size_t)blockIdx.y * A.N + i) * k + a] = same;
                total[h] += eterm;
            } else {
                total[h] += eterm - fmin(q, same);
            }
        }
    }
    red[threadIdx.x] = total[0];
    red[256 + threadIdx.x] = total[1];
    __syncthreads();
    if (slot == 0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int a = a0 + h * KP;
            if (a >= k) continue;
            double s = 0.0;
            for (int j = 0; j < slots; ++j) s += red[h * 256 + j * KP + a0];
            A.corr[((size_t)blockIdx.y * A.n_ppieces + blockIdx.x) * k + a] = s;
        }
    }
}

// out[col][a][b] = sum over the pieces, in piece order, of the partials (+ the parents' diagonal terms)
static __global__ void __launch_bounds__(256) expected_reduce_kernel(PmlExpArgs A) {
    const int k = A.k;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= k * k) return;
    const double* part = A.partial + (size_t)blockIdx.y * A.n_pieces * k * k + idx;
    double s = 0.0;
    for (int j = 0; j < A.n_pieces; ++j) s += part[(size_t)j * k * k];
    const int a = idx / k, b = idx % k;
    if (a == b) {
        const double* corr = A.corr + (size_t)blockIdx.y * A.n_ppieces * k + a;
        double d = 0.0;
        for (int j = 0; j < A.n_ppieces; ++j) d += corr[(size_t)j * k];
        s += d;
    }
    A.out[(size_t)blockIdx.y * k * k + idx] = s;
}
