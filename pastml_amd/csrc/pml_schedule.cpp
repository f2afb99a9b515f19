// Host-side planning of the tree schedules (pml_schedule.h).
#include "pml_schedule.h"
#include "pml_columns.h"   // pml_bu_lanes

#include <algorithm>
#include <cstdarg>
#include <cstdio>

static std::string message(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static std::string message(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}

// host-side validation of everything the kernels index with (a bad index would fault the GPU)
std::string pml_check_tree(const PmlTreeArrays& t) {
    const int n_nodes = t.n_nodes, n_roots = t.n_roots, n_bu_levels = t.n_bu_levels, n_td_levels = t.n_td_levels;
    const int *parent = t.parent, *first_child = t.first_child, *n_children = t.n_children, *bu_offsets = t.bu_offsets,
              *bu_order = t.bu_order, *td_offsets = t.td_offsets, *td_parent_offsets = t.td_parent_offsets,
              *td_parents = t.td_parents, *post_rank = t.post_rank;
    if (n_nodes <= 0 || n_roots <= 0 || n_roots > n_nodes) return "bad node/root counts";
    if (!parent || !first_child || !n_children || !t.dist || !bu_offsets || !td_offsets || !td_parent_offsets || !post_rank)
        return "NULL tree array";
    if (n_bu_levels < 0 || n_td_levels < 1) return "bad level counts";
    int n_internal = 0;
    for (int i = 0; i < n_nodes; ++i) {
        const int nc = n_children[i];
        if (nc < 0) return message("n_children[%d] < 0", i);
        if (nc > 0) {
            ++n_internal;
            const long long fc = first_child[i];
            if (fc <= i || fc + nc > n_nodes) return message("children of node %d out of range", i);
            for (int j = 0; j < nc; ++j)
                if (parent[fc + j] != i) return message("parent/child arrays disagree at node %d", i);
        }
        if (i < n_roots ? parent[i] != -1 : (parent[i] < 0 || parent[i] >= i))
            return message("parent[%d] = %d is not valid for level-ordered ids", i, parent[i]);
        if (!(t.dist[i] >= 0.0)) return message("dist[%d] is negative or NaN", i);
        if (post_rank[i] < 0 || post_rank[i] >= n_nodes) return message("post_rank[%d] out of range", i);
    }
    if (bu_offsets[0] != 0 || bu_offsets[n_bu_levels] != n_internal)
        return message("bu_offsets must cover the %d internal nodes", n_internal);
    if (td_parent_offsets[0] != 0 || td_parent_offsets[n_td_levels] != n_internal)
        return message("td_parent_offsets must cover the %d internal nodes", n_internal);
    if (td_offsets[0] != 0 || td_offsets[1] != n_roots || td_offsets[n_td_levels] != n_nodes)
        return "td_offsets must start with the roots and cover all nodes";
    if (n_internal > 0 && (!bu_order || !td_parents)) return "NULL level array";
    std::vector<char> seen(n_nodes, 0);
    std::vector<int> height(n_nodes, 0);
    for (int l = 0; l < n_bu_levels; ++l) {
        if (bu_offsets[l + 1] < bu_offsets[l]) return "bu_offsets not monotone";
        for (int q = bu_offsets[l]; q < bu_offsets[l + 1]; ++q) {
            const int n = bu_order[q];
            if (n < 0 || n >= n_nodes || n_children[n] == 0 || seen[n])
                return message("bu_order[%d] = %d is not a distinct internal node", q, n);
            seen[n] = 1;
            // every internal child must sit in an earlier level
            for (int j = 0; j < n_children[n]; ++j) {
                const int ch = first_child[n] + j;
                if (n_children[ch] > 0 && (!seen[ch] || height[ch] >= l + 1))
                    return message("bu level %d: node %d precedes its child %d", l, n, ch);
            }
            height[n] = l + 1;
        }
    }
    std::fill(seen.begin(), seen.end(), 0);
    for (int l = 0; l < n_td_levels; ++l) {
        if (td_parent_offsets[l + 1] < td_parent_offsets[l] || td_offsets[l + 1] < td_offsets[l]) return "td offsets not monotone";
        for (int q = td_parent_offsets[l]; q < td_parent_offsets[l + 1]; ++q) {
            const int n = td_parents[q];
            if (n < td_offsets[l] || n >= td_offsets[l + 1] || n_children[n] == 0 || seen[n])
                return message("td_parents[%d] = %d is not a distinct internal node of depth %d", q, n, l);
            seen[n] = 1;
        }
    }
    return "";
}

// ---------------------------------------------------------------------------------------------------------------------
// Node kinds under cherry fusion (a cherry: an internal node that is not a root and whose children are all tips; with
// fusion off every internal node is stored) and fused heights (a stored node: 1 + the largest fused height of its stored
// children; 0 for tips and cherries).  Independent of the numbering.  Returns the largest fused height.
static int kinds_and_heights(int N, const int* parent, const int* first_child, const int* n_children, bool fuse,
                             std::vector<unsigned char>& kind, std::vector<int>& fh) {
    kind.assign(N, PML_KIND_TIP);
    fh.assign(N, 0);
    for (int i = 0; i < N; ++i) {
        if (n_children[i] == 0) continue;
        bool all_tips = true;
        for (int j = 0; j < n_children[i]; ++j) all_tips &= n_children[first_child[i] + j] == 0;
        kind[i] = fuse && all_tips && parent[i] >= 0 ? PML_KIND_CHERRY : PML_KIND_STORED;
    }
    int max_h = 0;
    for (int i = N - 1; i >= 0; --i) {  // children have larger ids than their parent
        if (kind[i] != PML_KIND_STORED) continue;
        int h = 0;
        for (int j = 0; j < n_children[i]; ++j) {
            const int ch = first_child[i] + j;
            if (kind[ch] == PML_KIND_STORED && fh[ch] > h) h = fh[ch];
        }
        fh[i] = h + 1;
        max_h = std::max(max_h, fh[i]);
    }
    return max_h;
}

// the packed word of node n's unit descriptor (PmlUnit); kind == nullptr: every internal child counts as stored
static int packed_word(const int* first_child, const int* n_children, const unsigned char* kind, int n) {
    const int nc = n_children[n];
    int packed = nc < 15 ? nc : 15;
    bool cherries_ok = true, stored_first_two_only = true;
    for (int j = 0; j < 4 && j < nc; ++j) {
        const int ch = first_child[n] + j;
        int code = n_children[ch] == 0 ? 0 : 1;
        if (kind && kind[ch] == PML_KIND_CHERRY) {
            if (n_children[ch] > 4) {
                cherries_ok = false;
                code = 2;
            } else {
                code = 1 + n_children[ch];
            }
        }
        packed |= code << (8 + 3 * j);
        if (j >= 2 && code == 1) stored_first_two_only = false;
    }
    if (cherries_ok) packed |= 1 << 4;
    if (stored_first_two_only) packed |= 1 << 5;
    return packed;
}

static int child_code(int packed, int j) { return (packed >> (8 + 3 * j)) & 7; }
static bool stored_child01(const PmlUnit& u) { return child_code(u.packed, 0) == 1 || child_code(u.packed, 1) == 1; }
static bool cherry_child01(const PmlUnit& u) { return child_code(u.packed, 0) >= 2 || child_code(u.packed, 1) >= 2; }

// per level of a unit list (offs): some unit has a stored node as child 0 or 1 (at least one entry)
static std::vector<char> stored_child01_levels(const std::vector<PmlUnit>& u, const int* offs, int n_levels) {
    std::vector<char> v(n_levels > 0 ? n_levels : 1, 0);
    for (int l = 0; l < n_levels; ++l)
        for (int q = offs[l]; q < offs[l + 1] && !v[l]; ++q) v[l] = stored_child01(u[q]);
    return v;
}

// unit descriptors of a node list (at least one element); use_kind = false: every internal child counts as stored
static std::vector<PmlUnit> describe(const PmlForest& f, const int* list, size_t count, bool use_kind) {
    std::vector<PmlUnit> out(count > 0 ? count : 1);
    for (size_t q = 0; q < count; ++q) {
        PmlUnit& u = out[q];
        u.n = list[q];
        u.fc = f.first_child[u.n];
        u.pad = 0;
        u.packed = packed_word(f.first_child.data(), f.n_children.data(), use_kind ? f.kind.data() : nullptr, u.n);
        for (int j = 0; j < 4; ++j) u.cfc[j] = j < f.n_children[u.n] ? f.first_child[u.fc + j] : 0;
    }
    return out;
}
static std::vector<PmlUnit> describe(const PmlForest& f, const std::vector<int>& list, bool use_kind = true) {
    return describe(f, list.data(), list.size(), use_kind);
}

// The units of every level (offs) sorted by shape, stable.  fh given: by (shape, fused height) -- the order in which
// height_order lays out the children of a depth's units (the top-down lists of a shape-ordered forest).
static bool shape_less(const PmlUnit& x, const PmlUnit& y) { return x.packed < y.packed; }
static std::vector<PmlUnit> units_by_shape(const std::vector<PmlUnit>& in, const std::vector<int>& offs, size_t count,
                                           const int* fh = nullptr) {
    auto less = [&](const PmlUnit& x, const PmlUnit& y) { return x.packed != y.packed ? x.packed < y.packed : fh && fh[x.n] < fh[y.n]; };
    std::vector<PmlUnit> out(in);
    for (size_t l = 0; l + 1 < offs.size(); ++l) {
        const size_t a = (size_t)offs[l], b = std::min((size_t)offs[l + 1], count);
        if (b > a + 1) std::stable_sort(out.begin() + a, out.begin() + b, less);
    }
    return out;
}
static bool in_shape_order(const std::vector<PmlUnit>& in, const std::vector<int>& offs, size_t count) {
    for (size_t l = 0; l + 1 < offs.size(); ++l) {
        const size_t a = (size_t)offs[l], b = std::min((size_t)offs[l + 1], count);
        if (b > a + 1 && !std::is_sorted(in.begin() + a, in.begin() + b, shape_less)) return false;
    }
    return true;
}

// depth of every node (td_offsets)
static std::vector<int> node_depths(const PmlForest& f) {
    std::vector<int> depth(f.N, 0);
    for (size_t l = 0; l + 1 < f.td_offsets.size(); ++l)
        for (int i = f.td_offsets[l]; i < f.td_offsets[l + 1]; ++i) depth[i] = (int)l;
    return depth;
}

// The two-level pattern at node i: two children that each carry two cherries of two tips, the ids of the four cherries
// and of the eight tips consecutive (as breadth-first numbering makes them).  On the topology alone: under cherry
// fusion these are exactly the two-level units.
static bool two_level_root(const int* fc, const int* nch, int i) {
    auto tips2 = [&](int x) { return nch[x] == 2 && nch[fc[x]] == 0 && nch[fc[x] + 1] == 0; };
    auto pair = [&](int x) { return nch[x] == 2 && tips2(fc[x]) && tips2(fc[x] + 1) && fc[fc[x] + 1] == fc[fc[x]] + 2; };
    if (nch[i] != 2) return false;
    const int a = fc[i], b = a + 1;
    return pair(a) && pair(b) && fc[b] == fc[a] + 2 && fc[fc[b]] == fc[fc[a]] + 4;
}

// Forests with many nodes of three or four children: 15 % of the nodes with a child that has children (what is a stored
// node under cherry fusion).  Independent of the numbering.
static bool has_polytomies(int N, const int* first_child, const int* n_children) {
    long long n_inner = 0, n34 = 0;
    for (int i = 0; i < N; ++i) {
        const int nc = n_children[i];
        bool inner = false;
        for (int j = 0; j < nc && !inner; ++j) inner = n_children[first_child[i] + j] > 0;
        if (!inner) continue;
        ++n_inner;
        n34 += nc == 3 || nc == 4;
    }
    return n_inner > 0 && n34 * 100 >= 15 * n_inner;
}

// ---------------------------------------------------------------------------------------------------------------------
// Height-ordered numbering (round 5).  The C-ABI asks for breadth-first ids -- roots first, the children of a node
// contiguous, every depth a contiguous id range -- which leaves the ORDER OF THE SIBLING GROUPS INSIDE A DEPTH free.  The
// sweeps walk the nodes by fused height (bottom-up) and gather, per unit, 8-byte scalars of the unit's children (E, S, mask,
// exponent) and of the tips under its cherry children; in plain breadth-first order the children of the units of ONE height
// are scattered over their depth, so every gathered scalar costs a 128-byte line of its own (a random 262 144-tip tree moved
// 28.8 GB per marginal pass where the schedule needs 22.2, profiles/r04b_*).  Here the sibling groups of a depth are ordered
// by the height class of the unit that gathers them -- a stored node's children by its fused height, the tips of a cherry by
// the fused height of the cherry's parent -- and, inside a class, in the order of their parents: the children of consecutive
// units of a level are then consecutive in memory.  Same tree, same arithmetic per node, same bits (the order of a node's own
// children is kept); k = 64: marginal pass 5.8 -> 5.2 ms, k = 12: 3.25 -> 2.48, k = 4: 2.39 -> 1.68 (262 144 random tips x 32
// characters, profiles/r05e_height_order.txt).  A balanced tree is in this order already.
// Returns false (and leaves the vectors empty) when the caller's numbering is the height order.
// ---------------------------------------------------------------------------------------------------------------------
// by_shape (round 6): inside a depth the sibling groups are ordered by (shape, height class) of the unit that gathers them instead of
// by the class alone -- the level launches of wide units walk their lists sorted by shape (units_by_shape), so only then are the
// children of CONSECUTIVE units of a launch consecutive in memory (the top-down lists are sorted by (shape, class) to match).
static bool height_order(const PmlTreeArrays& t, bool fuse, bool by_shape, std::vector<int>& old_of_new, std::vector<int>& new_of_old) {
    const int N = t.n_nodes;
    const int *parent = t.parent, *first_child = t.first_child, *n_children = t.n_children;
    old_of_new.clear();
    new_of_old.clear();
    std::vector<unsigned char> kind;
    std::vector<int> fh;
    kinds_and_heights(N, parent, first_child, n_children, fuse, kind, fh);
    // the class of a sibling group: the fused height of the unit that gathers it (a cherry's parent for the tips of a
    // cherry; a cherry is never a root) -- and its shape, describe's packed word of that unit
    std::vector<long long> key(N, 0);
    for (int i = 0; i < N; ++i) {
        if (n_children[i] == 0) continue;
        const int unit = kind[i] == PML_KIND_STORED ? i : parent[i];
        key[i] = fh[unit];
        if (by_shape) key[i] |= (long long)packed_word(first_child, n_children, kind.data(), unit) << 32;
    }
    std::vector<int> order;
    order.reserve(N);
    for (int i = 0; i < t.n_roots; ++i) order.push_back(i);
    size_t lo = 0;
    bool identity = true;
    std::vector<int> par;
    for (int d = 0; d + 1 < t.n_td_levels; ++d) {
        const size_t hi = order.size();
        par.clear();
        for (size_t q = lo; q < hi; ++q)
            if (n_children[order[q]] > 0) par.push_back(order[q]);
        std::stable_sort(par.begin(), par.end(), [&](int x, int y) { return key[x] < key[y]; });
        for (int p : par)
            for (int j = 0; j < n_children[p]; ++j) {
                identity = identity && first_child[p] + j == (int)order.size();
                order.push_back(first_child[p] + j);
            }
        lo = hi;
    }
    if (identity || (int)order.size() != N) return false;
    old_of_new.swap(order);
    new_of_old.assign(N, 0);
    for (int q = 0; q < N; ++q) new_of_old[old_of_new[q]] = q;
    return true;
}

// t's arrays in the numbering num holds; t is pointed at them
static void renumber(PmlTreeArrays& t, PmlNumbering& num) {
    const int N = t.n_nodes, n_internal = t.bu_offsets[t.n_bu_levels];
    const std::vector<int>& o = num.old_of_new;
    const std::vector<int>& nw = num.new_of_old;
    num.parent.resize(N);
    num.first_child.resize(N);
    num.n_children.resize(N);
    num.post_rank.resize(N);
    num.dist.resize(N);
    for (int q = 0; q < N; ++q) {
        const int old = o[q];
        num.parent[q] = t.parent[old] >= 0 ? nw[t.parent[old]] : -1;
        num.n_children[q] = t.n_children[old];
        // (a tip's entry is never read; it only has to pass for an id)
        num.first_child[q] = t.n_children[old] > 0 ? nw[t.first_child[old]] : 0;
        num.post_rank[q] = t.post_rank[old];
        num.dist[q] = t.dist[old];
    }
    num.bu_order.assign(n_internal > 0 ? n_internal : 1, 0);
    num.td_parents.assign(n_internal > 0 ? n_internal : 1, 0);
    for (int l = 0; l < t.n_bu_levels; ++l) {
        for (int q = t.bu_offsets[l]; q < t.bu_offsets[l + 1]; ++q) num.bu_order[q] = nw[t.bu_order[q]];
        std::sort(num.bu_order.begin() + t.bu_offsets[l], num.bu_order.begin() + t.bu_offsets[l + 1]);
    }
    for (int l = 0; l < t.n_td_levels; ++l) {
        for (int q = t.td_parent_offsets[l]; q < t.td_parent_offsets[l + 1]; ++q) num.td_parents[q] = nw[t.td_parents[q]];
        std::sort(num.td_parents.begin() + t.td_parent_offsets[l], num.td_parents.begin() + t.td_parent_offsets[l + 1]);
    }
    t.parent = num.parent.data();
    t.first_child = num.first_child.data();
    t.n_children = num.n_children.data();
    t.post_rank = num.post_rank.data();
    t.dist = num.dist.data();
    t.bu_order = num.bu_order.data();
    t.td_parents = num.td_parents.data();
}

PmlForest pml_plan_forest(PmlTreeArrays& t, const PmlTune& tune, bool fuse, PmlNumbering& num) {
    PmlForest f;
    f.polytomies = has_polytomies(t.n_nodes, t.first_child, t.n_children);
    // Shape-aware order (round 6) for large forests without many polytomies: there the level launches walk shape-sorted lists
    // and a depth's sibling groups follow them.  Measured, marginal pass, class-only -> shape-aware numbering, bits unchanged
    // (profiles/r06q_shape_order.txt): random binary 262 144 tips x 32, k = 64 5.07 -> 4.94 ms, k = 12 2.29 -> 2.07, k = 8 1.91 ->
    // 1.68, k = 4 1.46 -> 1.35 (the last two with their lists sorted by shape as well, which the old numbering punished);
    // forests with polytomies lose 2 - 3 % (many shapes: short runs) and 40 000-tip trees 3 %: they keep the class-only order.
    bool shape_order = t.n_nodes >= 150000 && !f.polytomies;
    if (tune.on(T_SHAPE_ORDER)) shape_order = tune.get(T_SHAPE_ORDER, 1) != 0;
    if (!tune.on(T_NO_HEIGHT_ORDER) && height_order(t, fuse, shape_order, num.old_of_new, num.new_of_old)) renumber(t, num);
    f.shape_ordered = shape_order && !num.old_of_new.empty();

    const int N = t.n_nodes;
    f.fuse = fuse;
    f.N = N;
    f.n_roots = t.n_roots;
    f.n_internal = t.bu_offsets[t.n_bu_levels];
    f.parent.assign(t.parent, t.parent + N);
    f.first_child.assign(t.first_child, t.first_child + N);
    f.n_children.assign(t.n_children, t.n_children + N);
    f.bu_offsets.assign(t.bu_offsets, t.bu_offsets + t.n_bu_levels + 1);
    f.td_offsets.assign(t.td_offsets, t.td_offsets + t.n_td_levels + 1);
    f.td_parent_offsets.assign(t.td_parent_offsets, t.td_parent_offsets + t.n_td_levels + 1);
    // the fused level lists: the stored nodes by fused height (level l = height l + 1) and by depth
    const int max_h = kinds_and_heights(N, t.parent, t.first_child, t.n_children, fuse, f.kind, f.fh);
    f.bu_offsets_f.assign(max_h + 1, 0);
    for (int i = 0; i < N; ++i)
        if (f.kind[i] == PML_KIND_STORED) ++f.bu_offsets_f[f.fh[i]];
    // count of height h (h >= 1) -> exclusive prefix
    for (int h = 1, run = 0; h <= max_h; ++h) {
        const int cnt = f.bu_offsets_f[h];
        f.bu_offsets_f[h - 1] = run;
        run += cnt;
        if (h == max_h) f.bu_offsets_f[max_h] = run;
    }
    f.order_f.resize(f.n_stored());
    std::vector<int> cursor(f.bu_offsets_f);
    for (int i = 0; i < N; ++i)
        if (f.kind[i] == PML_KIND_STORED) f.order_f[cursor[f.fh[i] - 1]++] = i;
    f.td_parent_offsets_f.assign(t.n_td_levels + 1, 0);
    for (int l = 0; l < t.n_td_levels; ++l) {
        for (int q = t.td_parent_offsets[l]; q < t.td_parent_offsets[l + 1]; ++q)
            if (f.kind[t.td_parents[q]] == PML_KIND_STORED) f.tdp.push_back(t.td_parents[q]);
        f.td_parent_offsets_f[l + 1] = (int)f.tdp.size();
    }
    // Balanced parts (pml_plan_columns: the lane shape of the bottom-up kernels) -- counted on the topology alone, whatever
    // the switches, so that the lane shape, and with it a column's bits, is a function of k and the forest.
    long long n_two = 0;
    for (int i = 0; i < N; ++i) n_two += two_level_root(t.first_child, t.n_children, i);
    f.balanced_parts = n_two > 0 && n_two * 32 >= f.n_internal;
    return f;
}

// ---------------------------------------------------------------------------------------------------------------------
// Joint sweep of the eigen models: tiers of subtree blocks over the thin levels of the plain bottom-up lists
static void plan_eigen_tiers(const PmlForest& f, const PmlTreeArrays& t, const PmlTune& tune, const PmlUnit& slack,
                             PmlTreePlan& P) {
    PmlEigenTiers& E = P.eig.s;
    const int n_bu_levels = t.n_bu_levels, *bu_offsets = t.bu_offsets, *bu_order = t.bu_order;
    const int thin = (int)tune.get(T_EIGJ_TIER_THIN, 4096);
    const int depth = std::max(2, (int)tune.get(T_EIGJ_TIER_DEPTH, 4));
    const int top_nodes = 48;
    int L0 = n_bu_levels;
    while (L0 > 0 && bu_offsets[L0] - bu_offsets[L0 - 1] <= thin) --L0;
    if (tune.on(T_NO_EIGJ_TIERS) || n_bu_levels - L0 < 6) return;
    std::vector<int> level_of(f.N, -1), block_of(f.N, -1);
    for (int l = 0; l < n_bu_levels; ++l)
        for (int q = bu_offsets[l]; q < bu_offsets[l + 1]; ++q) level_of[bu_order[q]] = l;
    auto level = [&](int n) { return level_of[n]; };
    int a = L0;
    // The depth of a tier is the largest (up to 12 levels) whose blocks still have at most 12 nodes per
    // level -- one pass of a workgroup per level step at k = 20 (three nodes per wavefront).  A
    // balanced binary tree gets tiers of four levels, ragged trees deeper ones (measured: HIV1C-shaped
    // and random 40 000-tip trees are 10 - 20 % faster with 6 - 8 levels than with 4, cfg3 slower).
    // PASTML_HIP_EIGJ_TIER_DEPTH fixes the depth.
    const bool fixed_depth = tune.on(T_EIGJ_TIER_DEPTH);
    while (a + 2 <= n_bu_levels && bu_offsets[a + 1] - bu_offsets[a] > top_nodes) {
        int use = 0, nb = 0;
        for (int dep = fixed_depth ? depth : 12; dep >= 2; --dep) {
            if (a + dep > n_bu_levels) {
                if (fixed_depth) break;
                continue;
            }
            const int b = a + dep;
            // block of a node: its highest ancestor below level b (higher levels come last in the list,
            // so walking it backwards meets parents before children)
            nb = 0;
            for (int q = bu_offsets[b]; q-- > bu_offsets[a];) {
                const int n = bu_order[q];
                const int p = f.parent[n];
                block_of[n] = (p >= 0 && level_of[p] >= 0 && level_of[p] < b) ? block_of[p] : nb++;
            }
            std::vector<int> cell((size_t)nb * dep, 0);
            int widest_cell = 0;
            for (int q = bu_offsets[a]; q < bu_offsets[b]; ++q) {
                const int n = bu_order[q];
                widest_cell = std::max(widest_cell, ++cell[(size_t)block_of[n] * dep + (level_of[n] - a)]);
            }
            if (widest_cell <= 12 || dep == 2 || fixed_depth) {
                use = dep;
                break;
            }
        }
        if (use == 0) break;
        const int b = a + use;
        E.tiers.push_back({(int)P.eig.t.start.size(), nb, use});
        std::vector<std::vector<int>> members(nb);   // (by level, bu_order inside a level)
        for (int q = bu_offsets[a]; q < bu_offsets[b]; ++q) members[block_of[bu_order[q]]].push_back(bu_order[q]);
        for (const std::vector<int>& mem : members) P.eig.t.add_cells(mem.data(), mem.size(), level, a, use);
        for (int l = a; l < b; ++l) E.widest = std::max(E.widest, bu_offsets[l + 1] - bu_offsets[l]);
        a = b;
    }
    if (E.tiers.empty()) return;
    P.eig.units = describe(f, P.eig.t.list, false);
    P.eig.units.push_back(slack);  // (slack: an empty level at the end of the table is still addressed)
    P.eig.t.list.push_back(slack.n);
    E.first_level = L0;
    E.top_level = a;
    E.ok = true;
}

// joint back-trace tiers: from the first depth of more than 1 024 nodes on, tiers of up to 10 depths whose subtrees keep
// at most 256 nodes per depth (one pass of a workgroup per step)
static void plan_backtrace_tiers(const PmlForest& f, const PmlTune& tune, PmlTreePlan& P) {
    PmlBacktraceTiers& B = P.bt.s;
    const std::vector<int>& td_offsets = f.td_offsets;
    const int n_td_levels = (int)td_offsets.size() - 1;
    int d1 = 1;
    while (d1 < n_td_levels && td_offsets[d1 + 1] - td_offsets[d1] <= 1024) ++d1;
    if (tune.on(T_NO_BT_TIERS) || n_td_levels - d1 < 2) return;
    const std::vector<int> depth_of = node_depths(f);
    auto depth = [&](int n) { return depth_of[n]; };
    std::vector<int> anc(f.N, 0), by_block;
    for (int da = d1; da < n_td_levels;) {
        // one counting pass over up to 10 depths: nodes per (subtree, depth), the widest cell of every
        // depth; the tier takes the depths before the first one that is too wide
        const int dmax = std::min(10, n_td_levels - da);
        const int nb = td_offsets[da + 1] - td_offsets[da];
        std::vector<int> cnt10((size_t)nb * dmax, 0), widest(dmax, 0);
        for (int i = td_offsets[da]; i < td_offsets[da + dmax]; ++i) {
            const int dd = depth_of[i] - da;
            anc[i] = dd == 0 ? i - td_offsets[da] : anc[f.parent[i]];
            widest[dd] = std::max(widest[dd], ++cnt10[(size_t)anc[i] * dmax + dd]);
        }
        int use = 1;
        while (use < dmax && widest[use] <= 256) ++use;
        B.tiers.push_back({(int)P.bt.t.start.size(), nb, use});
        // the tier's nodes by subtree (ascending ids inside one: ascending depth), then per subtree its depth offsets
        std::vector<int> at(nb + 1, 0);
        for (int bl = 0; bl < nb; ++bl)
            for (int d = 0; d < use; ++d) at[bl + 1] += cnt10[(size_t)bl * dmax + d];
        for (int bl = 0; bl < nb; ++bl) at[bl + 1] += at[bl];
        by_block.resize(at[nb]);
        std::vector<int> cursor(at.begin(), at.end() - 1);
        for (int i = td_offsets[da]; i < td_offsets[da + use]; ++i) by_block[cursor[anc[i]]++] = i;
        for (int bl = 0; bl < nb; ++bl) P.bt.t.add_cells(by_block.data() + at[bl], at[bl + 1] - at[bl], depth, da, use);
        da += use;
    }
    P.bt.t.list.push_back(0);
    B.first_depth = d1;
    B.ok = true;
}

// ---- two-level units: stored nodes with two stored children that are each the parent of two cherries of two tips (ids of
// the four cherries and of the eight tips consecutive, as breadth-first numbering makes them); stacked units; the rest lists
static void plan_super(const PmlForest& f, const PmlTune& tune, PmlTreePlan& P) {
    PmlSuperSchedule& U = P.sup.s;
    const std::vector<int>&off = f.bu_offsets_f, &order = f.order_f, &fh = f.fh, &fc = f.first_child, &nch = f.n_children;
    const std::vector<unsigned char>& kind = f.kind;
    const int N = f.N, max_h = f.max_h(), n_stored = f.n_stored(), n_td_levels = (int)f.td_offsets.size() - 1;
    if (!f.fuse || tune.on(T_NO_SUPER)) return;
    std::vector<char> gone(N, 0);
    std::vector<int> sup_list;
    for (int i = 0; i < N; ++i)
        if (two_level_root(fc.data(), nch.data(), i)) sup_list.push_back(i);
    const bool env_min = tune.on(T_SUPER_MIN);
    const int min_units = (int)tune.get(T_SUPER_MIN, 64);
    // (a launch of its own per sweep: only where it carries a share of the work)
    // (PASTML_HIP_SUPER_MIN given: whatever their share, for tests on ragged forests)
    if (!((int)sup_list.size() >= min_units && (env_min || (long long)sup_list.size() * 16 >= n_stored)))
        sup_list.clear();   // (too few: no launch of their own; the stacked units below may still pay)
    for (int n : sup_list) gone[n] = gone[fc[n]] = gone[fc[n] + 1] = 1;
    // (the rest-list schedule needs wide units and a forest beyond the subtree blocks' reach to be used at all:
    // super_sweeps; here only the tree is known)
    if (n_stored == 0) return;
    PmlUnit pad;   // (padding element of the lists below when there are no two-level units)
    pad.n = order[0];
    pad.fc = fc[order[0]];
    pad.packed = pad.pad = 0;
    pad.cfc[0] = pad.cfc[1] = pad.cfc[2] = pad.cfc[3] = 0;
    P.sup.units.assign(std::max<size_t>(1, sup_list.size()), pad);
    for (size_t q = 0; q < sup_list.size(); ++q) {
        PmlUnit& u = P.sup.units[q];
        u.n = sup_list[q];
        u.fc = fc[u.n];
        u.packed = PML_PACKED_TWO_STORED;
        u.cfc[0] = fc[u.fc];
        u.cfc[1] = fc[u.fc + 1];
        u.pad = fc[u.cfc[0]];
    }
    // stacked units: ascending height, a node takes its two children over when both are plain units (not
    // two-level nodes, not taken over, not stacked themselves) with two stored children whose vectors are in
    // memory; only on levels of 1 024 .. 65 536 nodes (below: the narrow end's single launch; above: the
    // streaming levels' other lane shape)
    std::vector<char> stacked(N, 0), taken(N, 0), novec(N, 0);
    std::vector<int> stack_list;
    // (PASTML_HIP_STACK_MIN: smallest level that gets stacked units -- tests on small forests)
    const int stack_min = (int)tune.get(T_STACK_MIN, 1024);
    if (!tune.on(T_NO_STACK)) {
        for (int n : sup_list) novec[fc[n]] = novec[fc[n] + 1] = 1;
        auto level_size = [&](int node) { return off[fh[node]] - off[fh[node] - 1]; };
        auto has_vec = [&](int g) { return kind[g] == PML_KIND_STORED && !novec[g]; };
        auto plain2 = [&](int ch) {
            return kind[ch] == PML_KIND_STORED && !gone[ch] && !stacked[ch] && !taken[ch] && nch[ch] == 2 && has_vec(fc[ch]) &&
                   has_vec(fc[ch] + 1) && level_size(ch) <= 65536;
        };
        for (int n : order) {
            if (gone[n] || taken[n] || nch[n] != 2 || level_size(n) < stack_min || level_size(n) > 65536) continue;
            const int a = fc[n], b = a + 1;
            if (!plain2(a) || !plain2(b)) continue;
            stacked[n] = 1;
            taken[a] = taken[b] = novec[a] = novec[b] = 1;
            stack_list.push_back(n);
        }
    }
    // (A level with stacked units costs a launch more per sweep: they pay where they take most of what the
    // two-level units leave -- the balanced part of a tree -- and not at a tenth of the nodes: a random binary
    // tree of 262 144 tips had 6 132 of them, 10 % of its stored nodes, and was 3 % slower with them.
    // PASTML_HIP_STACK_MIN given: whatever their share.)
    if (!tune.on(T_STACK_MIN) && (long long)stack_list.size() * 3 * 2 < (long long)n_stored - 3 * (long long)sup_list.size())
        stack_list.clear();
    std::vector<int> stack_children, sup_children;
    for (int n : stack_list) {
        gone[n] = gone[fc[n]] = gone[fc[n] + 1] = 1;
        stack_children.push_back(fc[n]);
        stack_children.push_back(fc[n] + 1);
    }
    if (!stack_list.empty()) {
        const std::vector<int> depth_of = node_depths(f);
        // by bottom-up level (stack_list is in that order already) and by depth
        U.stack_bu_offsets.assign(max_h + 1, 0);
        for (int n : stack_list) ++U.stack_bu_offsets[fh[n]];
        for (int l = 0; l < max_h; ++l) U.stack_bu_offsets[l + 1] += U.stack_bu_offsets[l];
        std::vector<int> by_depth(stack_list);
        std::stable_sort(by_depth.begin(), by_depth.end(), [&](int x, int y) { return depth_of[x] < depth_of[y]; });
        U.stack_td_offsets.assign(n_td_levels + 1, 0);
        for (int n : by_depth) ++U.stack_td_offsets[depth_of[n] + 1];
        for (int l = 0; l < n_td_levels; ++l) U.stack_td_offsets[l + 1] += U.stack_td_offsets[l];
        P.sup.stack_bu = describe(f, stack_list);
        P.sup.stack_td = describe(f, by_depth);
        P.sup.stack_children = describe(f, stack_children);
        U.n_stack = (int)stack_list.size();
        // the chained top-down launch: the deepest stacked depth, when its grandchildren are the two-level nodes in list order
        int deepest = n_td_levels - 1;
        while (deepest >= 0 && U.stack_td_offsets[deepest + 1] == U.stack_td_offsets[deepest]) --deepest;
        const int a = U.stack_td_offsets[deepest], cnt = U.stack_td_offsets[deepest + 1] - a;
        bool lined_up = (long long)cnt * 4 == (long long)sup_list.size();
        for (int m = 0; m < cnt && lined_up; ++m) {
            const int n = by_depth[a + m], g0 = fc[fc[n]], g1 = fc[fc[n] + 1];
            lined_up = sup_list[4 * m] == g0 && sup_list[4 * m + 1] == g0 + 1 && sup_list[4 * m + 2] == g1 &&
                       sup_list[4 * m + 3] == g1 + 1;
        }
        if (lined_up) U.chain_depth = deepest;
        // the chained bottom-up launch: the lowest level with stacked units, under the same condition on its range of stack_list
        int lowest = 0;
        while (lowest < max_h && U.stack_bu_offsets[lowest + 1] == U.stack_bu_offsets[lowest]) ++lowest;
        const int b = U.stack_bu_offsets[lowest], bcnt = U.stack_bu_offsets[lowest + 1] - b;
        lined_up = (long long)bcnt * 4 == (long long)sup_list.size();
        for (int m = 0; m < bcnt && lined_up; ++m) {
            const int n = stack_list[b + m], g0 = fc[fc[n]], g1 = fc[fc[n] + 1];
            // (and all of one depth: balanced trees of different heights line up by height but not by depth -- such a forest keeps
            // the two launches in both sweeps)
            lined_up = sup_list[4 * m] == g0 && sup_list[4 * m + 1] == g0 + 1 && sup_list[4 * m + 2] == g1 &&
                       sup_list[4 * m + 3] == g1 + 1 && depth_of[n] == depth_of[stack_list[b]];
        }
        if (lined_up) U.bu_chain_level = lowest;
        if (tune.on(T_DEBUG))
            fprintf(stderr, "pastml_hip: %d stacked units, chain depth %d, bottom-up chain level %d\n", U.n_stack, U.chain_depth,
                    U.bu_chain_level);
    }
    if (sup_list.empty() && stack_list.empty()) return;   // (the plain level lists, nothing to build)
    // rest lists: the level structure of the fused lists, without the nodes the two-level units take over
    std::vector<int> bu_r, td_r;
    U.bu_offsets_r.assign(1, 0);
    for (int l = 0; l < max_h; ++l) {
        for (int q = off[l]; q < off[l + 1]; ++q)
            if (!gone[order[q]]) bu_r.push_back(order[q]);
        U.bu_offsets_r.push_back((int)bu_r.size());
    }
    U.td_offsets_r.assign(1, 0);
    for (int l = 0; l < n_td_levels; ++l) {
        for (int q = f.td_parent_offsets_f[l]; q < f.td_parent_offsets_f[l + 1]; ++q)
            if (!gone[f.tdp[q]]) td_r.push_back(f.tdp[q]);
        U.td_offsets_r.push_back((int)td_r.size());
    }
    for (int n : sup_list) {
        sup_children.push_back(fc[n]);
        sup_children.push_back(fc[n] + 1);
    }
    U.n_child_units = (int)sup_children.size();
    P.sup.child_units = describe(f, sup_children);  // (at least one element)
    P.sup.bu_units_r = describe(f, bu_r);
    P.sup.td_units_r = describe(f, td_r);
    U.bu_level_vec_r = stored_child01_levels(P.sup.bu_units_r, U.bu_offsets_r.data(), max_h);
    // (one element of slack: the walk over a level table reads the descriptor at a level's start even when
    // the level is empty)
    P.sup.bu_units_r.resize(bu_r.size() + 1, P.sup.units[0]);
    P.sup.td_units_r.resize(td_r.size() + 1, P.sup.units[0]);
    if (P.shape_sort) {
        P.sup.bu_units_rs = units_by_shape(P.sup.bu_units_r, U.bu_offsets_r, bu_r.size());
        P.sup.td_units_rs = units_by_shape(P.sup.td_units_r, U.td_offsets_r, td_r.size(), f.shape_ordered ? fh.data() : nullptr);
    }
    P.sup.lists = true;
    U.n = (int)sup_list.size();
    // worth its lists: two-level units, or stacked units that take a sixteenth of the stored nodes over
    U.ok = U.n > 0 || U.n_stack >= 64 || (U.n_stack > 0 && tune.on(T_STACK_MIN));
    if (tune.on(T_DEBUG))
        fprintf(stderr, "pastml_hip: %d two-level units (%d of %d stored nodes)%s\n", U.n, 3 * U.n, n_stored,
                U.ok ? "" : " -- plain level lists");
}

// ---- subtree blocks: stored nodes -> blocks (maximal subtrees of <= S stored nodes) + top
static void plan_blocks(const PmlForest& f, const PmlTune& tune, PmlTreePlan& P) {
    PmlBlockSchedule& B = P.blocks.s;
    const std::vector<int>&off = f.bu_offsets_f, &order = f.order_f, &fh = f.fh, &parent = f.parent, &tdp = f.tdp;
    const int N = f.N, max_h = f.max_h(), n_stored = f.n_stored(), n_td_levels = (int)f.td_offsets.size() - 1;
    const int S = (int)tune.get(T_BLOCK_NODES, 256);  // measured: 128-512 are within a few per cent, 1024+ loses at k >= 16
    const int cap_stored = (int)tune.get(T_BLOCK_MAX_STORED, 1 << 17);  // beyond: the streaming level kernels
    if (!(S > 0 && n_stored > S && n_stored <= cap_stored)) return;
    auto stored = [&](int i) { return f.kind[i] == PML_KIND_STORED; };
    std::vector<int> ssz(N, 0), blk(N, -1);
    const std::vector<int> depth = node_depths(f);
    for (int i = N - 1; i >= 0; --i) {
        if (!stored(i)) continue;
        ssz[i] += 1;
        if (parent[i] >= 0) ssz[parent[i]] += ssz[i];
    }
    // Height cap.  All blocks run in one launch and the top starts after it: a sweep costs (levels of the
    // tallest block) + (levels of the top).  Ragged trees have thin subtrees of few nodes and many levels;
    // uncapped, such a block outlasts all others while the top's lowest levels wait for it (HIV1C: 47 + 27
    // level steps for a tree of 57 levels).  Blocks therefore end below the lowest level of the top: what
    // sticks out joins levels the top walks anyway, and blocks + top together are as many level steps as
    // the forest has levels.  (PASTML_HIP_BLOCK_HEIGHT_CAP: 0 = no cap, n = cap at fused height n.)
    int h_cap = max_h;
    for (int n : order)
        if (ssz[n] > S) h_cap = std::min(h_cap, fh[n]);
    if (tune.on(T_BLOCK_HEIGHT_CAP)) {
        const int v = (int)tune.get(T_BLOCK_HEIGHT_CAP, 0);
        h_cap = v > 0 ? v : max_h + 1;
    }
    int nb = 0;
    for (int i = 0; i < N; ++i) {  // parents have smaller ids
        if (!stored(i) || ssz[i] > S || fh[i] >= h_cap) continue;
        const int p = parent[i];
        blk[i] = (p >= 0 && blk[p] >= 0) ? blk[p] : nb++;
    }
    // per block: its nodes by fused height (bottom-up) and by depth (top-down), each as consecutive levels
    std::vector<std::vector<int>> members(nb);
    for (int i = 0; i < N; ++i)
        if (blk[i] >= 0) members[blk[i]].push_back(i);
    for (std::vector<int>& mem : members) {  // ascending ids = non-decreasing depth
        P.blocks.td.add_runs(mem.data(), mem.size(), [&](int n) { return depth[n]; });
        std::stable_sort(mem.begin(), mem.end(), [&](int x, int y) { return fh[x] < fh[y]; });
        P.blocks.bu.add_runs(mem.data(), mem.size(), [&](int n) { return fh[n]; });
    }
    // the top: stored nodes outside the blocks, by fused height / by depth
    std::vector<int> top_bu, top_td;
    B.top_bu_offsets.assign(1, 0);
    for (int l = 0; l < max_h; ++l) {
        for (int q = off[l]; q < off[l + 1]; ++q)
            if (blk[order[q]] < 0) top_bu.push_back(order[q]);
        if ((int)top_bu.size() > B.top_bu_offsets.back()) B.top_bu_offsets.push_back((int)top_bu.size());
    }
    B.top_td_offsets.assign(n_td_levels + 1, 0);
    for (int l = 0; l < n_td_levels; ++l) {
        for (int q = f.td_parent_offsets_f[l]; q < f.td_parent_offsets_f[l + 1]; ++q)
            if (blk[tdp[q]] < 0) top_td.push_back(tdp[q]);
        B.top_td_offsets[l + 1] = (int)top_td.size();
    }
    const int n_top_levels = (int)B.top_bu_offsets.size() - 1;
    if (nb == 0 || n_top_levels + 1 >= max_h) return;  // (no fewer dependent launches than the level schedule)
    P.blocks.bu_units = describe(f, P.blocks.bu.list);
    P.blocks.td_units = describe(f, P.blocks.td.list);
    P.blocks.top_bu_units = describe(f, top_bu);
    P.blocks.top_td_units = describe(f, top_td);
    if (!tune.on(T_NO_SHAPE_SORT)) {
        // inside every level by shape (a wave of one shape runs that shape's code only: walk_levels); the
        // blocks' level tables lie one behind the other, so the whole array delimits the segments
        P.blocks.bu_units = units_by_shape(P.blocks.bu_units, P.blocks.bu.lv, P.blocks.bu.list.size());
        P.blocks.td_units = units_by_shape(P.blocks.td_units, P.blocks.td.lv, P.blocks.td.list.size());
        P.blocks.top_bu_units = units_by_shape(P.blocks.top_bu_units, B.top_bu_offsets, top_bu.size());
        P.blocks.top_td_units = units_by_shape(P.blocks.top_td_units, B.top_td_offsets, top_td.size());
    }
    B.top_bu_vec = stored_child01_levels(P.blocks.top_bu_units, B.top_bu_offsets.data(), n_top_levels);
    B.n_blocks = nb;
    for (int l : P.blocks.bu.levels) B.steps += l;
    if (tune.on(T_DEBUG))
        fprintf(stderr, "pastml_hip: %d stored nodes, %d subtree blocks, %lld block levels, %d top levels of %d\n", n_stored,
                nb, B.steps, n_top_levels, max_h);
    B.ok = true;
}

PmlTreePlan pml_plan_tree(const PmlForest& f, const PmlTreeArrays& t, const PmlTune& tune) {
    PmlTreePlan P;
    const int n_stored = f.n_stored();
    for (int i = 0; i < f.N; ++i) {
        if (f.n_children[i] == 0) P.tips.push_back(i);
        if (f.kind[i] == PML_KIND_CHERRY) P.cherries.push_back(i);
    }
    // unit descriptors (PmlUnit) for the node lists the F81 kernels walk
    P.cherry_units = describe(f, P.cherries, false);
    P.bu_units_f = describe(f, f.order_f);
    P.bu_level_vec_f = stored_child01_levels(P.bu_units_f, f.bu_offsets_f.data(), f.max_h());
    P.td_units_f = describe(f, f.tdp);
    P.td_cherry_prefix.assign(n_stored + 1, 0);
    for (int q = 0; q < n_stored; ++q) P.td_cherry_prefix[q + 1] = P.td_cherry_prefix[q] + cherry_child01(P.td_units_f[q]);
    P.bu_units = describe(f, t.bu_order, f.n_internal, false);
    plan_eigen_tiers(f, t, tune, P.bu_units[0], P);
    P.bu_level_vec = stored_child01_levels(P.bu_units, t.bu_offsets, t.n_bu_levels);
    plan_backtrace_tiers(f, tune, P);
    // Units of one shape next to each other.  Within a level the order of the units is free, and a wavefront runs
    // the union of its units' control flow: on a balanced tree every unit of a level has the same kinds of children
    // (tip / stored node / cherry of m tips), on a ragged one a wave of 8 units met most combinations and ran them
    // one after the other.  For the level launches of wide units (8 states per lane: 32 < k <= 64) every level's
    // units are sorted by the descriptor's shape word -- stable, ids ascend inside a shape, neighbours still read
    // neighbouring memory.  262 144-tip random binary tree x 32 characters, k = 64: marginal pass 6.5 -> 5.7 ms;
    // 100 000 tips with polytomies: 2.86 -> 2.13 ms; narrow units (k = 4: 64 units per wave, every lane its own
    // rows) lose 20 % to the scattered rows and keep id order.  PASTML_HIP_NO_SHAPE_SORT: id order everywhere.
    // (a balanced tree is in shape order as it is: no second copy, the launches walk the id-ordered lists)
    P.shape_sort = !tune.on(T_NO_SHAPE_SORT) && n_stored > 0 &&
                   !(in_shape_order(P.bu_units_f, f.bu_offsets_f, n_stored) && in_shape_order(P.td_units_f, f.td_parent_offsets_f, n_stored));
    if (P.shape_sort) {
        // top-down lists: by (shape, height class) -- the order in which height_order lays the children of a depth's units
        // out (bottom-up lists are per class already)
        P.bu_units_fs = units_by_shape(P.bu_units_f, f.bu_offsets_f, n_stored);
        P.td_units_fs = units_by_shape(P.td_units_f, f.td_parent_offsets_f, n_stored, f.shape_ordered ? f.fh.data() : nullptr);
    }
    plan_super(f, tune, P);
    plan_blocks(f, tune, P);
    // (the thin ends of a large forest are cut into subtree blocks when the columns are known: pml_plan_thin_ends)
    P.small = f.N <= (int)tune.get(T_SMALL_MAX_NODES, 2048);
    return P;
}

// ---- thin ends of a large forest (thin_bottom_up / deep_top_down).
// A ragged forest has many levels that hold a few hundred to a few thousand units: a launch of its own costs
// 5 - 15 us each, a level step inside a workgroup's walk 2 us.  Bottom-up, the thin levels are the high ones
// (every fused level from floor_level on holds at most THIN_UNITS units): subtree blocks + top over that part
// of the forest, the blocks in ONE launch behind the wide levels' launches, the top in the narrow end's launch.
// Top-down, they are the deep ones: the subtrees hanging at first_depth in ONE launch behind the wide depths.
// Small subtrees share a workgroup (bins of up to THIN_BLOCK_NODES units; units of one level of different
// subtrees do not depend on each other), so a workgroup's waves have work.
static void plan_thin_bottom_up(const PmlForest& f, const PmlTune& tune, int thin, int S, int narrow, PmlThinPlan& P) {
    PmlThinSchedule& H = P.thin;
    const std::vector<int>&off = f.bu_offsets_f, &order = f.order_f, &fh = f.fh, &parent = f.parent;
    const int N = f.N, max_h = f.max_h(), n_stored = f.n_stored();
    // levels [L0, Ltop) are thin and not yet narrow
    int L0 = max_h, Ltop = max_h;
    while (L0 > 0 && off[L0] - off[L0 - 1] <= thin) --L0;
    while (Ltop > L0 && off[Ltop] - off[Ltop - 1] <= narrow) --Ltop;
    if (!(thin > 0 && L0 > 0 && Ltop - L0 >= 3)) return;
    std::vector<int> ssz(N), blk(N);
    int a = L0;
    while (a < Ltop) {
        // the tier's nodes: fused height in (a, hc), hc = the lowest height at which a subtree of them exceeds S
        std::fill(ssz.begin(), ssz.end(), 0);
        for (int i = N - 1; i >= 0; --i) {
            if (f.kind[i] != PML_KIND_STORED || fh[i] <= a) continue;
            ssz[i] += 1;
            if (parent[i] >= 0) ssz[parent[i]] += ssz[i];
        }
        int hc = max_h + 1;
        for (int q = off[a]; q < n_stored; ++q)
            if (ssz[order[q]] > S) hc = std::min(hc, fh[order[q]]);
        // subtrees into bins: the open one while it fits (parents have smaller ids)
        std::fill(blk.begin(), blk.end(), -1);
        int nb = 0, fill = 0;
        for (int i = 0; i < N; ++i) {
            if (f.kind[i] != PML_KIND_STORED || fh[i] <= a || fh[i] >= hc) continue;
            const int p = parent[i];
            if (p >= 0 && blk[p] >= 0) {
                blk[i] = blk[p];
            } else {
                if (nb == 0 || fill + ssz[i] > S) {
                    ++nb;
                    fill = 0;
                }
                fill += ssz[i];
                blk[i] = nb - 1;
            }
        }
        std::vector<std::vector<int>> members(nb);
        for (int q = off[a]; q < off[hc - 1]; ++q) members[blk[order[q]]].push_back(order[q]);   // (ascending height)
        H.tiers.push_back({(int)P.bu.start.size(), nb});
        for (const std::vector<int>& mem : members) P.bu.add_runs(mem.data(), mem.size(), [&](int n) { return fh[n]; });
        if (tune.on(T_DEBUG))
            fprintf(stderr, "pastml_hip: thin bottom-up tier: levels %d .. %d of %d, %d units in %d bins\n", a, hc - 2, max_h,
                    off[hc - 1] - off[a], nb);
        a = hc - 1;
    }
    if ((int)H.tiers.size() + 2 > a - L0) return;   // (no launches saved)
    P.bu_units = describe(f, P.bu.list);
    if (!tune.on(T_NO_SHAPE_SORT)) P.bu_units = units_by_shape(P.bu_units, P.bu.lv, P.bu.list.size());
    P.bu_units.push_back(P.bu_units[0]);  // (slack: walk_levels fetches a level's first unit before it looks at its size)
    H.floor_level = L0;
    H.top_level = a;
    H.ok = true;
}

// top-down: the depths behind the widest one
static void plan_thin_top_down(const PmlForest& f, const PmlTune& tune, int thin, int S, int narrow, PmlThinPlan& P) {
    PmlDeepSchedule& D = P.deep;
    const std::vector<int>&toff = f.td_parent_offsets_f, &tdp = f.tdp, &parent = f.parent;
    const int n_td_levels = (int)toff.size() - 1, n_stored = f.n_stored();
    int widest = 0;
    for (int l = 1; l < n_td_levels; ++l)
        if (toff[l + 1] - toff[l] > toff[widest + 1] - toff[widest]) widest = l;
    int D0 = n_td_levels;
    while (D0 > widest + 1 && toff[D0] - toff[D0 - 1] <= thin) --D0;
    int n_mid = 0;
    for (int l = D0; l < n_td_levels; ++l) n_mid += toff[l + 1] - toff[l] > narrow;
    if (!(thin > 0 && D0 > 0 && D0 < n_td_levels && n_mid >= 3)) return;
    // a unit's bin: that of its parent's unit; the units of depth D0 open the subtrees
    std::vector<int> bin(f.N, -1), size(f.N, 0);
    for (int q = n_stored - 1; q >= toff[D0]; --q) {   // (the lists ascend in depth: children come later)
        const int n = tdp[q];
        size[n] += 1;
        if (q >= toff[D0 + 1]) size[parent[n]] += size[n];
    }
    int nb = 0, fill = 0;
    for (int q = toff[D0]; q < toff[D0 + 1]; ++q) {
        const int n = tdp[q];
        if (nb == 0 || fill + size[n] > S) {
            ++nb;
            fill = 0;
        }
        fill += size[n];
        bin[n] = nb - 1;
    }
    std::vector<std::vector<int>> members(nb);
    for (int q = toff[D0]; q < n_stored; ++q) {
        const int n = tdp[q];
        if (q >= toff[D0 + 1]) bin[n] = bin[parent[n]];
        members[bin[n]].push_back(n);   // (ascending depth)
    }
    const std::vector<int> depth = node_depths(f);
    for (const std::vector<int>& mem : members) P.td.add_runs(mem.data(), mem.size(), [&](int n) { return depth[n]; });
    P.td_units = describe(f, P.td.list);
    if (!tune.on(T_NO_SHAPE_SORT)) P.td_units = units_by_shape(P.td_units, P.td.lv, P.td.list.size());
    P.td_units.push_back(P.td_units[0]);
    D.first_depth = D0;
    D.n_blocks = nb;
    D.ok = true;
    if (tune.on(T_DEBUG))
        fprintf(stderr, "pastml_hip: thin top-down depths from %d of %d: %d units in %d bins\n", D0, n_td_levels,
                (int)P.td.list.size(), nb);
}

PmlThinPlan pml_plan_thin_ends(const PmlForest& f, const PmlTune& tune, int thin) {
    PmlThinPlan P;
    if (f.max_h() <= 0) return P;
    const int S = std::max(8, (int)tune.get(T_THIN_BLOCK_NODES, 256));
    const int narrow = std::min(128, std::max(1, thin / 32));  // (levels of about this many units are the single-workgroup launch's anyway)
    plan_thin_bottom_up(f, tune, thin, S, narrow, P);
    plan_thin_top_down(f, tune, thin, S, narrow, P);
    return P;
}

// ---------------------------------------------------------------------------------------------------------------------
// The sweeps' launch sequences (pml_schedule.h, PmlLaunch)
// ---------------------------------------------------------------------------------------------------------------------
// The narrow end of a large forest (the levels near the roots hold a handful of nodes each) is walked by ONE launch
// with a workgroup barrier between levels instead of one latency-bound launch per level: returns the number of
// consecutive levels, counted from the root end, that hold at most `limit` units each (0 if fewer than two do).
// Measured on MI355X: with one column (cfg2, 65 536 tips) 512 units per level is the best cut (0.205 -> 0.181 ms per
// marginal pass); one workgroup per column walks the levels, so with many columns the level kernels, which spread a
// level over the whole chip, win earlier: the limit shrinks with the number of columns.
// The fused eigen sweeps pass their own limit: a pass of theirs is a ~10 us dependent chain, so only levels that one
// workgroup finishes in a single pass per wave belong to the narrow end.
static int narrow_levels(const PmlSweepTraits& t, const std::vector<int>& off, int n_levels, bool from_front, int C, int fixed_limit = 0,
                         int top_down = -1, int skip = 0) {
    if (t.wide_states) return 0;   // (no multi-level kernels beyond 256 states)
    int limit = fixed_limit > 0 ? fixed_limit : (t.narrow_units > 0 ? t.narrow_units : std::max(8, 512 / std::max(1, C)));
    if (fixed_limit <= 0 && t.narrow_units <= 0 && t.f81) {
        // ... but never below half a pass of the walking workgroup (512 threads, g lanes per unit): such a level is one
        // wavefront's work per SIMD either way, and a launch of its own costs 5 - 10 us where a level step inside the
        // walk costs 2.  Random 262 144-tip tree x 32 characters, marginal pass: k = 4 1.66 -> 1.52 ms, k = 12 2.56 -> 2.37,
        // k = 64 unchanged (profiles/r05j_narrow_units.txt, r05l_narrow_ab.txt); same bits (PmlColumnPlan::bu_shape).
        const bool td = top_down < 0 ? from_front : top_down != 0;   // (which sweep's lane shape walks the levels)
        const int g = td ? t.Gt : pml_bu_lanes(t.bu_wide_lanes, t.Gf);
        limit = std::max(limit, 256 / std::max(1, g));
    }
    int n = 0;
    for (int q = 0; q < n_levels; ++q) {
        const int l = skip + (from_front ? q : n_levels - 1 - q);
        if (off[l + 1] - off[l] > limit) break;
        ++n;
    }
    return n >= 2 ? n : 0;
}
// the run of narrow depths right below the roots (td_offsets[d] .. td_offsets[d + 1] = the nodes of depth d; the roots are depth 0)
static int narrow_depths(const PmlSweepTraits& t, const PmlForest& f, int limit) {
    return narrow_levels(t, f.td_offsets, (int)f.td_offsets.size() - 2, true, t.C, limit, -1, 1);
}

namespace {
struct Plan {
    std::vector<PmlLaunch> v;
    int branch = 0, bracket = PML_NO_BRACKET;
    PmlLaunch& add(int op, int list = L_NONE, int first = 0, int count = 0, int kind = 0) {
        v.push_back(PmlLaunch{(unsigned char)op, (unsigned char)list, (unsigned char)kind, (unsigned char)bracket,
                              (unsigned char)branch, false, true, first, count, 0});
        return v.back();
    }
    // a launch per level l0 .. l1 - 1 of an offsets table; an empty level keeps its record (the launcher returns at once and the
    // profile counts it) or is skipped; after(l): what else level l launches
    template <class K, class A>
    void levels(int op, int list, const std::vector<int>& off, int l0, int l1, bool keep_empty, K kind, A after) {
        for (int l = l0; l < l1; ++l) {
            if (keep_empty || off[l + 1] > off[l]) add(op, list, off[l], off[l + 1] - off[l], kind(l));
            after(l);
        }
    }
    template <class K>
    void levels(int op, int list, const std::vector<int>& off, int l0, int l1, bool keep_empty, K kind) {
        levels(op, list, off, l0, l1, keep_empty, kind, [](int) {});
    }
};
const auto no_kind = [](int) { return 0; };
const auto td_fused_kind = [](int) { return (int)SW_TD_FUSED; };
}  // namespace

// the stacked units of level / depth l, if any
static void add_stack(Plan& p, const PmlSuperSchedule& U, const std::vector<int>& off, int l) {
    if (U.n_stack > 0 && off[l + 1] > off[l]) p.add(OP_STACK, L_NONE, l, off[l + 1] - off[l]);
}

// Bottom-up sweep of an eigen model: the tips, then the levels -- the thin ones in tiers of subtree blocks where the forest has
// them (pml_ctx::EigenTiers; only while their levels are thin for the whole batch: with many columns a level fills the chip),
// what is left above the tiers a launch each while wider than `wide` (a forest of many trees), then the narrow end in one launch
// (E: the tiers, or null where the sweep has none)
static void eigen_bottom_up(Plan& p, const PmlForest& f, const PmlSweepTraits& t, int family, const PmlEigenTiers* E, int wide,
                            int narrow_limit) {
    const int nb = (int)f.bu_offsets.size() - 1;
    const auto fam = [family](int) { return family; };
    p.add(OP_EIG_TIPS, L_NONE, 0, 0, family);
    if (E != nullptr) {
        p.levels(OP_EIG_LEVEL, L_BU_PLAIN, f.bu_offsets, 0, E->first_level, true, fam);
        for (size_t q = 0; q < E->tiers.size(); ++q) p.add(OP_EIG_TIER, L_NONE, (int)q, E->tiers[q].n_blocks, family);
        int l = E->top_level;
        while (l < nb && f.bu_offsets[l + 1] - f.bu_offsets[l] > wide) ++l;
        p.levels(OP_EIG_LEVEL, L_BU_PLAIN, f.bu_offsets, E->top_level, l, true, fam);
        p.add(OP_EIG_NARROW, L_BU_PLAIN, l, nb - l, family);   // (counted by the profile even where no level is left for it)
        return;
    }
    const int tail = narrow_levels(t, f.bu_offsets, nb, false, t.C, narrow_limit);
    p.levels(OP_EIG_LEVEL, L_BU_PLAIN, f.bu_offsets, 0, nb - tail, true, fam);
    if (tail > 0) p.add(OP_EIG_NARROW, L_BU_PLAIN, nb - tail, tail, family);
}

std::vector<PmlLaunch> pml_plan_bottom_up(const PmlForest& f, const PmlSchedules& s, const PmlSweepTraits& t, bool is_marginal) {
    const bool eig = t.eigen_fused, gemm = is_marginal && t.eigen_gemm, eigj = !is_marginal && t.eigen_joint_valu;
    const bool fused = is_marginal && t.f81;
    Plan p;
    p.branch = fused ? (t.single_launch ? BU_ONE_LAUNCH : t.blocks ? BU_BLOCKS : t.super ? BU_SUPER : t.thin ? BU_THIN : BU_FUSED)
               : (t.f81 && t.fuse && !t.has_init && t.n_cherries > 0 && t.W == 1) ? BU_FUSED_JOINT
               : eigj ? BU_EIGJ : gemm ? BU_GEMM : eig ? BU_EIG_FUSED : BU_PLAIN;
    // (eigen tiers only while their levels are thin for the whole batch: with many columns a level fills the chip)
    const bool tiers = s.eig->ok && (long long)s.eig->widest * t.C <= 16384 && !(gemm && !eigj && t.no_eigg_tiers);
    if (tiers && p.branch == BU_EIGJ) p.branch = BU_EIGJ_TIERS;
    if (tiers && p.branch == BU_GEMM) p.branch = BU_GEMM_TIERS;
    if (p.branch != BU_ONE_LAUNCH) {  // the single-launch kernel resets the error words itself
        p.add(OP_RESET_ERR).arg = eigj ? 1 : 0;
        // the fused eigen sweeps build P(t) themselves, the two-GEMM sweeps never need it
        if (!eig && !gemm && !eigj && !t.hky_fused) p.add(OP_PREP);
    }
    p.bracket = 0;
    const int nl = (int)f.bu_offsets_f.size() - 1;
    const int fused_list = t.level_lists_sorted ? L_BU_FUSED_SORTED : L_BU_FUSED;
    auto marg_kind = [](const std::vector<char>& vec) {
        return [&vec](int l) { return (int)(vec[l] ? SW_BU_MARG_FUSED : SW_BU_MARG_FUSED_NOVEC); };
    };
    // the levels next to the roots and ln L in one launch: the last of the sweep, outside the profile's bracket
    auto narrow_end = [&](int list, int first_level, int tail) {
        p.bracket = PML_NO_BRACKET;
        if (tail > 0) p.add(OP_LEVELS, list, first_level, tail).signal = t.sched_cols <= 64 && !t.no_spin_wait;
    };
    switch (p.branch) {
        case BU_ONE_LAUNCH: {   // prep + every level + ln L in one launch
            PmlLaunch& r = p.add(OP_LEVELS, L_BU_FUSED, 0, nl);
            r.arg = 1;
            r.signal = t.sched_cols <= 64 && !t.no_spin_wait;
            break;
        }
        case BU_BLOCKS: {   // subtree blocks in one launch, then the top part: level launches, its narrow end (and ln L) in one launch
            const PmlBlockSchedule& B = *s.blocks;
            p.add(OP_BLOCKS, L_NONE, 0, B.n_blocks);
            const int n = (int)B.top_bu_offsets.size() - 1;
            const int tail = narrow_levels(t, B.top_bu_offsets, n, false, t.sched_cols);
            p.levels(OP_LEVEL, L_TOP_BU, B.top_bu_offsets, 0, n - tail, true, marg_kind(B.top_bu_vec));
            narrow_end(L_TOP_BU, n - tail, tail);
            break;
        }
        case BU_SUPER: {   // the two-level units first (they depend on tips only), then the levels of what is left
            const PmlSuperSchedule& U = *s.sup;
            // (bu_chain: the stacked units of bu_chain_level run inside the two-level launch, which hands them their grandchildren's
            // vectors through LDS -- all of them two-level nodes, so the launch at the front of the sweep has what they need; no
            // record of their own, the opening record says which level it carries)
            const int chained = t.bu_chain && U.n > 0 ? U.bu_chain_level : -1;
            p.bracket = 4;
            if (U.n > 0) p.add(OP_SUPER, L_NONE, 0, U.n).arg = chained + 1;
            p.bracket = 0;
            const int n = (int)U.bu_offsets_r.size() - 1;
            int tail = narrow_levels(t, U.bu_offsets_r, n, false, t.sched_cols);
            // (the narrow end's single launch walks the rest lists only: it starts above the last level with stacked units)
            for (int l = n - 1; l >= 0 && U.n_stack > 0; --l)
                if (U.stack_bu_offsets[l + 1] > U.stack_bu_offsets[l]) {
                    tail = std::min(tail, n - 1 - l);
                    break;
                }
            if (tail < 2) tail = 0;
            // (a level's stacked units read vectors of two levels down: independent of the level's own launch)
            p.levels(OP_LEVEL, t.level_lists_sorted ? L_REST_BU_SORTED : L_REST_BU, U.bu_offsets_r, 0, n - tail, false,
                     marg_kind(U.bu_level_vec_r), [&](int l) { if (l != chained) add_stack(p, U, U.stack_bu_offsets, l); });
            narrow_end(L_REST_BU, n - tail, tail);
            break;
        }
        case BU_THIN: {
            // the wide levels one launch each, the thin ones in tiers of subtree blocks (a launch per tier), then the narrow
            // end's single launch (in between, level launches where a level is still too wide for it)
            const PmlThinSchedule& H = *s.thin;
            p.levels(OP_LEVEL, fused_list, f.bu_offsets_f, 0, H.floor_level, true, marg_kind(*s.bu_level_vec_f));
            for (size_t q = 0; q < H.tiers.size(); ++q) p.add(OP_BLOCKS, L_NONE, 1 + (int)q, H.tiers[q].n_blocks);
            const int tail = std::min(nl - H.top_level, narrow_levels(t, f.bu_offsets_f, nl, false, t.sched_cols));
            p.levels(OP_LEVEL, fused_list, f.bu_offsets_f, H.top_level, nl - tail, true, marg_kind(*s.bu_level_vec_f));
            narrow_end(L_BU_FUSED, nl - tail, tail);
            break;
        }
        case BU_FUSED: {
            const int tail = narrow_levels(t, f.bu_offsets_f, nl, false, t.sched_cols);
            p.levels(OP_LEVEL, fused_list, f.bu_offsets_f, 0, nl - tail, true, marg_kind(*s.bu_level_vec_f));
            narrow_end(L_BU_FUSED, nl - tail, tail);
            break;
        }
        case BU_FUSED_JOINT:   // joint sweep over the cherry-fused lists (no altered nodes whose tables would need rewriting)
            p.levels(OP_LEVEL, L_BU_FUSED, f.bu_offsets_f, 0, nl, true,
                     [&](int l) { return (int)((*s.bu_level_vec_f)[l] ? SW_BU_JOINT_FUSED : SW_BU_JOINT_FUSED_NOVEC); });
            break;
        case BU_EIGJ_TIERS:
        case BU_EIGJ:   // joint sweep of an eigen model on the vector units (pml_kernels_eigen_joint.h)
            eigen_bottom_up(p, f, t, EIG_JOINT, tiers ? s.eig : nullptr, 48, t.waves * (64 / t.k));
            break;
        case BU_GEMM_TIERS:
        case BU_GEMM:
            // marginal sweep: P(t) is never formed, msg = A (e o (A^-1 v)) as two small GEMMs per 16 nodes; levels one
            // workgroup finishes in a pass or two per wave (4 waves x 16 nodes) share one launch
            eigen_bottom_up(p, f, t, EIG_GEMM, tiers ? s.eig : nullptr, 2 * t.waves * 16, 2 * t.waves * 16);
            break;
        case BU_EIG_FUSED:   // every node once, in the launch of its level: the tips first, then the internal nodes by height
            eigen_bottom_up(p, f, t, EIG_FUSED, nullptr, 0, t.waves * t.eig_nb);
            break;
        default:
            p.levels(OP_LEVEL, L_BU_PLAIN, f.bu_offsets, 0, (int)f.bu_offsets.size() - 1, true, [&](int l) {
                return (int)(is_marginal ? SW_BU_MARG : (t.f81 && !(*s.bu_level_vec)[l] ? SW_BU_JOINT_NOVEC : SW_BU_JOINT));
            });
    }
    p.bracket = PML_NO_BRACKET;
    if (p.v.back().op != OP_LEVELS) p.add(OP_LOGLIK);   // (the launch that walks the last levels writes ln L itself)
    return p.v;
}

// Top-down sweep of an eigen model below the roots: the run of narrow depths in one launch, then a launch per depth
static void eigen_top_down(Plan& p, const PmlForest& f, const PmlSweepTraits& t, int family, int limit) {
    const int head = narrow_depths(t, f, limit);
    if (head > 0) p.add(OP_EIG_NARROW, L_IDS, 1, head, family);
    p.levels(OP_EIG_LEVEL, L_IDS, f.td_offsets, 1 + head, (int)f.td_offsets.size() - 1, false, [family](int) { return family; });
}

std::vector<PmlLaunch> pml_plan_top_down(const PmlForest& f, const PmlSchedules& s, const PmlSweepTraits& t, bool wants_signal) {
    const int nd = (int)f.td_offsets.size() - 1;
    const bool td_small = t.single_launch && t.f81;
    const bool levels_f81 = t.f81 && !td_small;
    const bool signal = wants_signal && t.C <= 64 && !t.no_spin_wait;   // (the last launch of the pass)
    Plan p;
    // the roots, or the roots and the `head` levels right below them in one launch
    auto roots = [&](int list, int head) {
        if (head == 0) p.add(OP_ROOTS, L_NONE, 0, t.n_roots);
        else p.add(OP_LEVELS, list, 0, head);
        p.bracket = 1;
    };
    if (levels_f81 && t.blocks) {
        // block schedule: the top part (roots, its narrow end in one launch, its wide levels one launch each),
        // then all subtree blocks in one launch
        const PmlBlockSchedule& B = *s.blocks;
        p.branch = TD_BLOCKS;
        const int head = t.n_roots <= 64 ? narrow_levels(t, B.top_td_offsets, nd, true, t.C) : 0;
        roots(L_TOP_TD, head);
        p.levels(OP_LEVEL, L_TOP_TD, B.top_td_offsets, head, nd, false, td_fused_kind);
        p.add(OP_BLOCKS, L_NONE, 0, B.n_blocks).signal = signal;
        return p.v;
    }
    if (levels_f81 && t.super) {
        // the levels of the rest lists, then every two-level unit in one launch (it needs its node's row only, and
        // that comes from a unit of the rest lists or from the roots)
        const PmlSuperSchedule& U = *s.sup;
        p.branch = TD_SUPER;
        int head = t.n_roots <= 64 ? narrow_levels(t, U.td_offsets_r, nd, true, t.C) : 0;
        // (... and the single launch below the roots ends above the first depth with stacked nodes)
        for (int l = 0; l < nd && U.n_stack > 0; ++l)
            if (U.stack_td_offsets[l + 1] > U.stack_td_offsets[l]) {
                head = std::min(head, l);
                break;
            }
        if (head < 2) head = 0;
        roots(L_REST_TD, head);
        // (the children of the stacked nodes of a depth: their rows come from the depth above)
        // (td_chain: the stacked units of chain_depth run inside the two-level launch, which takes their grandchildren's
        // rows from LDS -- no record of their own, the closing record says which depth it carries)
        const int chained = t.td_chain && U.n > 0 ? U.chain_depth : -1;
        p.levels(OP_LEVEL, t.level_lists_sorted ? L_REST_TD_SORTED : L_REST_TD, U.td_offsets_r, head, nd, false, td_fused_kind,
                 [&](int l) { if (l != chained) add_stack(p, U, U.stack_td_offsets, l); });
        p.bracket = 3;
        if (U.n > 0) p.add(OP_SUPER, L_NONE, 0, U.n).arg = chained + 1;
        return p.v;
    }
    // F81 family: the roots and the levels right below them in one launch
    const int head = (levels_f81 && t.n_roots <= 64) ? narrow_levels(t, f.td_parent_offsets_f, nd, true, t.C) : 0;
    const bool deep = levels_f81 && t.deep && s.deep->first_depth > head;
    p.branch = td_small ? TD_ONE_LAUNCH : deep ? TD_DEEP : t.eigen_gemm ? TD_GEMM : t.eigen_fused ? TD_EIG_FUSED : TD_LEVELS;
    if (td_small) p.bracket = 1;
    else roots(L_TD_FUSED, head);
    if (td_small) p.add(OP_LEVELS, L_TD_FUSED, 0, nd).signal = signal;
    // eigen models, child-centric: the nodes of a depth are a contiguous id range (roots are depth 0, done above)
    else if (t.eigen_gemm) eigen_top_down(p, f, t, EIG_GEMM, 2 * t.waves * 16);
    else if (t.eigen_fused) eigen_top_down(p, f, t, EIG_FUSED, t.waves * t.eig_nb);
    if (p.branch != TD_LEVELS && p.branch != TD_DEEP) return p.v;
    const int fused_list = t.level_lists_sorted ? L_TD_FUSED_SORTED : L_TD_FUSED;
    // the staging hint of a level of the whole forest's fused list
    auto hint = [&](size_t from) {
        const std::vector<int>& pre = *s.td_cherry_prefix;
        for (size_t i = from; i < p.v.size(); ++i) {
            const size_t a = (size_t)p.v[i].first, b = a + (size_t)p.v[i].count;
            if (!pre.empty() && b < pre.size()) p.v[i].cherries = pre[b] != pre[a];
        }
    };
    // F81 family: the thin depths at the DEEP end of a ragged forest (a handful of parents each) in one launch as well
    // -- a launch of their own costs 9 - 11 us each, a level step of the walk 2 - 3 (round 5) --, and when many of the deep
    // depths are thin, all of them: the subtrees hanging at the first one, a workgroup per (bin of subtrees, column)
    // walking its depths (pml_plan_thin_ends)
    const size_t from = p.v.size();
    if (deep) {
        p.levels(OP_LEVEL, fused_list, f.td_parent_offsets_f, head, s.deep->first_depth, false, td_fused_kind);
        hint(from);
        p.add(OP_BLOCKS, L_NONE, 1, s.deep->n_blocks);
        return p.v;
    }
    int tail = 0;
    // (units of fewer than 8 lanes only: at k = 64 a level step inside the walk costs what the launch does)
    if (t.f81 && t.Gt < 8 && !t.no_td_tail) {
        tail = std::min(nd - head, narrow_levels(t, f.td_parent_offsets_f, nd, false, t.C, 0, 1));
        if (tail < 2) tail = 0;
    }
    if (t.f81) {
        p.levels(OP_LEVEL, fused_list, f.td_parent_offsets_f, head, nd - tail, false, td_fused_kind);
        hint(from);
    } else {
        p.levels(OP_LEVEL, L_TD_PLAIN, f.td_parent_offsets, head, nd, false, [](int) { return (int)SW_TD; });
    }
    p.bracket = PML_NO_BRACKET;
    if (tail > 0) p.add(OP_LEVELS, L_TD_FUSED, nd - tail, tail).arg = 1;
    return p.v;
}

// the back-trace launches: the narrow depths below the roots in one launch, the wide ones one launch each or in tiers
std::vector<PmlLaunch> pml_plan_backtrace(const PmlForest& f, const PmlSchedules& s, const PmlSweepTraits& t, int* head_out) {
    const int head = narrow_depths(t, f, 1024);
    const PmlBacktraceTiers& B = *s.bt;
    // (tiers while one column's narrow end is the limit they were cut for: with many columns the narrow end is shorter
    // and the depths in between keep their launches)
    bool tiers = B.ok && 1 + head >= B.first_depth;
    for (const PmlBacktraceTiers::Tier& T : B.tiers)
        tiers = tiers && (long long)T.n_blocks * t.C <= 8192;  // (a workgroup per subtree and column: only while few)
    Plan p;
    p.branch = tiers ? BT_TIERS : BT_LEVELS;
    if (head > 0) p.add(OP_BT_NARROW, L_IDS, 1, tiers ? B.first_depth - 1 : head);
    if (tiers)
        for (size_t q = 0; q < B.tiers.size(); ++q) p.add(OP_BT_TIER, L_NONE, (int)q, B.tiers[q].n_blocks);
    else
        p.levels(OP_BT_LEVEL, L_IDS, f.td_offsets, 1 + head, (int)f.td_offsets.size() - 1, false, no_kind);
    if (head_out) *head_out = head;
    return p.v;
}

PmlSweepOutcome pml_plan_outcome(const std::vector<PmlLaunch>& plan) {
    PmlSweepOutcome o;
    for (const PmlLaunch& r : plan) o.n_signals += r.signal ? 1 : 0;
    o.final_signals = o.n_signals > 0;   // (only a plan's last launch signals)
    o.fused_joint = !plan.empty() && plan.front().branch == BU_FUSED_JOINT;
    return o;
}
