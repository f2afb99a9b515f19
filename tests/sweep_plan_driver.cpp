// Host-only check of the sweeps' launch plans (pastml_amd/csrc/pml_schedule.h): plans forests with pml_schedule.cpp and, over
// a grid of PmlSweepTraits, checks every plan for coverage, order, once-only launches, the per-bracket launch counts and the
// outcome the host keeps of it (pml_plan_outcome).
// Built and run by tests/test_sweep_plan_host.py; prints FAIL lines and exits 1, or one OK line.
#include "../pastml_amd/csrc/pml_schedule.h"

#include <algorithm>
#include <cstdio>
#include <functional>
#include <random>
#include <set>

static int g_failures = 0;
static std::string g_case;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++g_failures <= 40) {                     \
                printf("FAIL [%s] ", g_case.c_str());     \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        }                                                 \
    } while (0)

// ---- forests: ids in breadth-first order, a node's children next to each other (what pml_tree_upload is given)
struct Tree {
    int n_roots = 0;
    std::vector<int> parent, first_child, n_children, post_rank, bu_offsets, bu_order, td_offsets, td_parent_offsets, td_parents;
    std::vector<double> dist;
};
// budgets: tips below each root; split(tips of a node) -> tips of its children
static Tree grow(const std::vector<int>& budgets, const std::function<std::vector<int>(int)>& split) {
    Tree T;
    T.n_roots = (int)budgets.size();
    std::vector<int> budget = budgets, depth(budgets.size(), 0);
    T.parent.assign(budgets.size(), -1);
    for (size_t i = 0; i < budget.size(); ++i) {
        T.first_child.push_back(0);
        T.n_children.push_back(0);
        if (budget[i] <= 1) continue;
        const std::vector<int> parts = split(budget[i]);
        T.first_child[i] = (int)budget.size();
        T.n_children[i] = (int)parts.size();
        for (int b : parts) {
            budget.push_back(b);
            depth.push_back(depth[i] + 1);
            T.parent.push_back((int)i);
        }
    }
    const int N = (int)budget.size();
    T.dist.assign(N, 1.0);
    T.post_rank.resize(N);
    std::vector<int> height(N, 0);
    int max_h = 0, max_d = 0;
    for (int i = N - 1; i >= 0; --i) {
        T.post_rank[i] = i;
        for (int j = 0; j < T.n_children[i]; ++j) height[i] = std::max(height[i], 1 + height[T.first_child[i] + j]);
        max_h = std::max(max_h, height[i]);
        max_d = std::max(max_d, depth[i]);
    }
    T.bu_offsets.assign(1, 0);
    for (int h = 1; h <= max_h; ++h) {
        for (int i = 0; i < N; ++i)
            if (height[i] == h) T.bu_order.push_back(i);
        T.bu_offsets.push_back((int)T.bu_order.size());
    }
    T.td_offsets.assign(1, 0);
    T.td_parent_offsets.assign(1, 0);
    for (int d = 0, i = 0; d <= max_d; ++d) {
        for (; i < N && depth[i] == d; ++i)
            if (T.n_children[i] > 0) T.td_parents.push_back(i);
        T.td_offsets.push_back(i);
        T.td_parent_offsets.push_back((int)T.td_parents.size());
    }
    return T;
}

static std::mt19937 g_rng(12345);
static std::vector<int> split_even(int n) { return {n - n / 2, n / 2}; }
static std::vector<int> split_comb(int n) { return {n - 1, 1}; }
static std::vector<int> split_random(int n) {
    const int a = 1 + (int)(g_rng() % (unsigned)(n - 1));
    return {a, n - a};
}
static std::vector<int> split_poly(int n) {   // 15 % of the nodes with three or four children
    const int want = (g_rng() % 100 < 15) ? 3 + (int)(g_rng() % 2) : 2;
    std::vector<int> parts(std::min(want, n), 1);
    for (int left = n - (int)parts.size(); left > 0; --left) ++parts[g_rng() % parts.size()];
    if (parts.size() == 2 && n > 2) return split_random(n);
    return parts;
}

// ---- a planned forest and what a launch record of it covers
struct Planned {
    PmlForest f;
    PmlNumbering num;
    PmlTreeArrays t;
    PmlTreePlan P;
    PmlThinPlan H;
    PmlSchedules S;
    int nd() const { return (int)f.td_offsets.size() - 1; }
};

static std::set<int> g_ops, g_branches;

static void block_nodes(const PmlLevelTable& t, int first_block, int n_blocks, std::vector<int>& out) {
    for (int g = first_block; g < first_block + n_blocks; ++g)
        for (int q = t.lv[t.start[g]]; q < t.lv[t.start[g] + t.levels[g]]; ++q) out.push_back(t.list[q]);
}

// the nodes a record computes (bottom-up: stored / internal nodes; top-down: parents, or nodes for L_IDS); multi: the launch
// orders its own nodes (levels with a barrier in between, or a unit that computes its children itself)
static std::vector<int> covered(const Planned& F, const PmlLaunch& r, bool bottom_up, bool& multi) {
    const PmlBlockSchedule& B = F.P.blocks.s;
    const PmlSuperSchedule& U = F.P.sup.s;
    std::vector<int> out;
    auto unit_nodes = [&](const std::vector<PmlUnit>& u, int a, int b) {
        for (int i = a; i < b; ++i) out.push_back(u[i].n);
    };
    auto list_nodes = [&](int list, int a, int b) {
        switch (list) {
            case L_BU_FUSED: case L_BU_FUSED_SORTED: out.insert(out.end(), F.f.order_f.begin() + a, F.f.order_f.begin() + b); break;
            case L_TD_FUSED: case L_TD_FUSED_SORTED: out.insert(out.end(), F.f.tdp.begin() + a, F.f.tdp.begin() + b); break;
            case L_BU_PLAIN: out.insert(out.end(), F.t.bu_order + a, F.t.bu_order + b); break;
            case L_TD_PLAIN: out.insert(out.end(), F.t.td_parents + a, F.t.td_parents + b); break;
            case L_TOP_BU: unit_nodes(F.P.blocks.top_bu_units, a, b); break;
            case L_TOP_TD: unit_nodes(F.P.blocks.top_td_units, a, b); break;
            case L_REST_BU: case L_REST_BU_SORTED: unit_nodes(F.P.sup.bu_units_r, a, b); break;
            case L_REST_TD: case L_REST_TD_SORTED: unit_nodes(F.P.sup.td_units_r, a, b); break;
            case L_IDS: for (int i = a; i < b; ++i) out.push_back(i); break;
            default: CHECK(false, "list %d of op %d has no nodes", list, r.op);
        }
    };
    auto offsets = [&](int list) -> const std::vector<int>& {
        switch (list) {
            case L_BU_FUSED: return F.f.bu_offsets_f;
            case L_TD_FUSED: return F.f.td_parent_offsets_f;
            case L_TOP_BU: return B.top_bu_offsets;
            case L_TOP_TD: return B.top_td_offsets;
            case L_REST_BU: return U.bu_offsets_r;
            case L_REST_TD: return U.td_offsets_r;
            case L_BU_PLAIN: return F.f.bu_offsets;
            default: return F.f.td_offsets;
        }
    };
    auto with_children = [&](const std::vector<PmlUnit>& u, int a, int b) {
        for (int i = a; i < b; ++i) {
            out.push_back(u[i].n);
            for (int j = 0; j < F.f.n_children[u[i].n]; ++j) out.push_back(F.f.first_child[u[i].n] + j);
        }
    };
    multi = true;
    switch (r.op) {
        case OP_LEVEL: case OP_EIG_LEVEL: case OP_BT_LEVEL:
            multi = false;
            list_nodes(r.list, r.first, r.first + r.count);
            break;
        case OP_LEVELS: case OP_EIG_NARROW: case OP_BT_NARROW: {
            const std::vector<int>& off = offsets(r.list);
            CHECK(r.first >= 0 && r.first + r.count < (int)off.size(), "levels %d + %d beyond the table", r.first, r.count);
            list_nodes(r.list, off[r.first], off[r.first + r.count]);
            break;
        }
        case OP_BLOCKS:
            if (r.first == 0) out = bottom_up ? F.P.blocks.bu.list : F.P.blocks.td.list;
            else if (bottom_up) block_nodes(F.H.bu, F.H.thin.tiers[r.first - 1].first_block, F.H.thin.tiers[r.first - 1].n_blocks, out);
            else out = F.H.td.list;
            break;
        case OP_SUPER: with_children(F.P.sup.units, 0, U.n); break;
        case OP_STACK: {
            const std::vector<int>& off = bottom_up ? U.stack_bu_offsets : U.stack_td_offsets;
            with_children(bottom_up ? F.P.sup.stack_bu : F.P.sup.stack_td, off[r.first], off[r.first + 1]);
            break;
        }
        case OP_EIG_TIER: block_nodes(F.P.eig.t, F.P.eig.s.tiers[r.first].first_block, F.P.eig.s.tiers[r.first].n_blocks, out); break;
        case OP_BT_TIER: block_nodes(F.P.bt.t, F.P.bt.s.tiers[r.first].first_block, F.P.bt.s.tiers[r.first].n_blocks, out); break;
        default: break;
    }
    return out;
}

// coverage (every node of the universe exactly once), order and the once-only launches of one plan
static void check_plan(const Planned& F, const std::vector<PmlLaunch>& plan, int dir /* 0 bottom-up, 1 top-down, 2 back-trace */,
                       bool fused_universe, long long count[5]) {
    const PmlForest& f = F.f;
    std::vector<int> done(f.N, -1);
    const bool by_id = !plan.empty() && (plan.back().list == L_IDS || plan.back().op == OP_BT_TIER || plan.back().op == OP_BT_NARROW);
    auto in_universe = [&](int n) {
        if (by_id) return f.parent[n] >= 0;
        return fused_universe ? f.kind[n] == PML_KIND_STORED : f.n_children[n] > 0;
    };
    int n_loglik = 0, n_signal = 0;
    std::fill(count, count + 5, 0);
    CHECK(!plan.empty(), "empty plan");
    for (size_t idx = 0; idx < plan.size(); ++idx) {
        const PmlLaunch& r = plan[idx];
        g_ops.insert(r.op);
        g_branches.insert(r.branch);
        CHECK(r.branch == plan[0].branch, "records of two branches in one plan");
        if (r.bracket != PML_NO_BRACKET) {
            CHECK(r.bracket < 5, "bracket %d", r.bracket);
            if (r.bracket < 5) ++count[r.bracket];
        }
        if (r.signal) {
            ++n_signal;
            CHECK(idx + 1 == plan.size(), "the launch that raises the completion word is not the last");
        }
        if (r.op == OP_LOGLIK || (dir == 0 && r.op == OP_LEVELS)) {
            ++n_loglik;
            CHECK(idx + 1 == plan.size(), "ln L is not written by the last launch");
        }
        bool multi = false;
        const std::vector<int> nodes = covered(F, r, dir == 0, multi);
        for (int n : nodes) {
            if (!in_universe(n)) continue;   // (a unit's tips and cherries)
            CHECK(done[n] < 0, "node %d covered by launches %d and %zu", n, done[n], idx);
            done[n] = (int)idx;
        }
        for (int n : nodes) {
            if (!in_universe(n)) continue;
            if (dir == 0) {   // children before parents
                for (int j = 0; j < f.n_children[n]; ++j) {
                    const int c = f.first_child[n] + j;
                    if (!in_universe(c)) continue;
                    CHECK(done[c] >= 0 && (done[c] < (int)idx || multi), "launch %zu (op %d) reads child %d of node %d before it is written", idx, r.op, c, n);
                }
            } else {          // parents before children
                const int p = f.parent[n];
                if (p < 0 || (by_id && f.parent[p] < 0)) continue;   // (the roots' rows: OP_ROOTS / the bottom-up sweep)
                CHECK(done[p] >= 0 && (done[p] < (int)idx || multi), "launch %zu (op %d) reads the row of node %d's parent %d before it is written", idx, r.op, n, p);
            }
        }
    }
    for (int n = 0; n < f.N; ++n)
        if (in_universe(n)) CHECK(done[n] >= 0, "node %d is covered by no launch", n);
    if (dir == 0) CHECK(n_loglik == 1, "ln L written %d times", n_loglik);
    CHECK(n_signal <= 1, "%d launches raise the completion word", n_signal);
}

// ---- the launch counts of the profile brackets as the sweeps computed them before the plans existed (prof_end's arithmetic)
static int nonempty(const std::vector<int>& off, int l0, int l1) {
    int n = 0;
    for (int l = l0; l < l1; ++l) n += off[l + 1] > off[l];
    return n;
}
static void expected_counts(const Planned& F, const std::vector<PmlLaunch>& plan, const PmlSweepTraits& t, long long want[5]) {
    const PmlForest& f = F.f;
    const PmlSuperSchedule& U = F.P.sup.s;
    const PmlBlockSchedule& B = F.P.blocks.s;
    std::fill(want, want + 5, 0);
    const int nl = (int)f.bu_offsets_f.size() - 1, nb = (int)f.bu_offsets.size() - 1, nd = F.nd();
    const PmlLaunch& last = plan.back().op == OP_LOGLIK ? plan[plan.size() - 2] : plan.back();
    const PmlLaunch& first = plan.front();
    // the narrow ends as planned: the tail of a bottom-up sweep, the head below the roots of a top-down one
    const int tail = (last.op == OP_LEVELS || last.op == OP_EIG_NARROW) ? last.count : 0;
    const int head = first.op == OP_LEVELS ? first.count : 0;
    switch (first.branch) {
        case BU_ONE_LAUNCH: want[0] = 1; break;
        case BU_BLOCKS: want[0] = 1 + ((int)B.top_bu_offsets.size() - 1) - tail; break;
        case BU_SUPER: {
            const int n = (int)U.bu_offsets_r.size() - 1;
            want[4] = U.n > 0 ? 1 : 0;
            want[0] = nonempty(U.bu_offsets_r, 0, n - tail) + (U.n_stack > 0 ? nonempty(U.stack_bu_offsets, 0, n - tail) : 0);
            break;
        }
        case BU_THIN: want[0] = F.H.thin.floor_level + (long long)F.H.thin.tiers.size() + (nl - tail - F.H.thin.top_level); break;
        case BU_FUSED: want[0] = nl - tail; break;
        case BU_FUSED_JOINT: want[0] = nl; break;
        case BU_EIGJ_TIERS: case BU_GEMM_TIERS: {
            const PmlEigenTiers& E = F.P.eig.s;
            const int wide = first.branch == BU_EIGJ_TIERS ? 48 : 2 * t.waves * 16;
            long long extra = 0;
            for (int l = E.top_level; l < nb && f.bu_offsets[l + 1] - f.bu_offsets[l] > wide; ++l) ++extra;
            want[0] = E.first_level + 2 + extra + (long long)E.tiers.size();
            break;
        }
        case BU_EIGJ: case BU_GEMM: case BU_EIG_FUSED: want[0] = nb + 1 - tail + (tail > 0 ? 1 : 0); break;
        case BU_PLAIN: want[0] = nb; break;
        case TD_ONE_LAUNCH: want[1] = 1; break;
        case TD_BLOCKS: want[1] = nonempty(B.top_td_offsets, head, nd) + 1; break;
        case TD_SUPER:
            want[1] = nonempty(U.td_offsets_r, head, nd) + (U.n_stack > 0 ? nonempty(U.stack_td_offsets, head, nd) : 0);
            want[3] = U.n > 0 ? 1 : 0;
            break;
        case TD_GEMM: case TD_EIG_FUSED: {
            const int h = plan.size() > 1 && plan[1].op == OP_EIG_NARROW ? plan[1].count : 0;
            want[1] = (h > 0 ? 1 : 0) + nonempty(f.td_offsets, 1 + h, nd);
            break;
        }
        case TD_DEEP: want[1] = nonempty(f.td_parent_offsets_f, head, F.H.deep.first_depth) + 1; break;
        case TD_LEVELS: {
            const int td_tail = last.op == OP_LEVELS && plan.size() > 1 ? last.count : 0;
            want[1] = nonempty(t.f81 ? f.td_parent_offsets_f : f.td_parent_offsets, head, nd - td_tail);
            break;
        }
        default: break;
    }
}

// ---- the rules of the narrow ends, the level kinds, the list choice, the staging hint and the completion word, restated
// the run of levels from the root end that hold at most the limit of units each (fewer than two: none)
static int narrow_ref(const PmlSweepTraits& t, const std::vector<int>& off, bool from_front, int C, bool top_down_shape) {
    if (t.wide_states) return 0;
    int limit = t.narrow_units > 0 ? t.narrow_units : std::max(8, 512 / std::max(1, C));
    if (t.narrow_units <= 0 && t.f81) limit = std::max(limit, 256 / (top_down_shape ? t.Gt : (t.bu_wide_lanes ? 8 : t.Gf)));
    const int n_levels = (int)off.size() - 1;
    int n = 0;
    while (n < n_levels) {
        const int l = from_front ? n : n_levels - 1 - n;
        if (off[l + 1] - off[l] > limit) break;
        ++n;
    }
    return n >= 2 ? n : 0;
}
static int level_of(const std::vector<int>& off, const PmlLaunch& r) {
    for (int l = 0; l + 1 < (int)off.size(); ++l)
        if (off[l] == r.first && off[l + 1] - off[l] == r.count) return l;
    return -1;
}
static void check_rules(const Planned& F, const std::vector<PmlLaunch>& plan, const PmlSweepTraits& t) {
    const PmlForest& f = F.f;
    const PmlSuperSchedule& U = F.P.sup.s;
    const PmlBlockSchedule& B = F.P.blocks.s;
    const int branch = plan.front().branch, nd = F.nd();
    const PmlLaunch& last = plan.back();
    const PmlLaunch& first = plan.front();
    const bool bu = branch <= BU_PLAIN;
    // the narrow ends
    const int tail = bu && last.op == OP_LEVELS ? last.count : 0;
    const int head = !bu && first.op == OP_LEVELS ? first.count : 0;
    if (branch == BU_FUSED) CHECK(tail == narrow_ref(t, f.bu_offsets_f, false, t.sched_cols, false), "tail %d", tail);
    if (branch == BU_BLOCKS) CHECK(tail == narrow_ref(t, B.top_bu_offsets, false, t.sched_cols, false), "top tail %d", tail);
    if (branch == BU_SUPER) {
        int want = narrow_ref(t, U.bu_offsets_r, false, t.sched_cols, false);
        const int n = (int)U.bu_offsets_r.size() - 1;
        for (int l = n - 1; l >= 0 && U.n_stack > 0; --l)
            if (U.stack_bu_offsets[l + 1] > U.stack_bu_offsets[l]) { want = std::min(want, n - 1 - l); break; }
        CHECK(tail == (want < 2 ? 0 : want), "rest tail %d, the rule gives %d", tail, want);
    }
    if (branch == TD_LEVELS || branch == TD_DEEP || branch == TD_BLOCKS || branch == TD_SUPER) {
        const std::vector<int>& off = branch == TD_BLOCKS ? B.top_td_offsets : branch == TD_SUPER ? U.td_offsets_r : f.td_parent_offsets_f;
        int want = (t.f81 && t.n_roots <= 64) ? narrow_ref(t, off, true, t.C, true) : 0;
        for (int l = 0; branch == TD_SUPER && l < nd && U.n_stack > 0; ++l)
            if (U.stack_td_offsets[l + 1] > U.stack_td_offsets[l]) { want = std::min(want, l); break; }
        if (want < 2) want = 0;
        CHECK(head == want, "head %d, the rule gives %d", head, want);
        CHECK((first.op == OP_ROOTS) == (want == 0), "the roots' launch with a head of %d", want);
        if (branch == TD_LEVELS) {
            int wt = 0;
            if (t.f81 && t.Gt < 8 && !t.no_td_tail) wt = std::min(nd - head, narrow_ref(t, f.td_parent_offsets_f, false, t.C, true));
            if (wt < 2) wt = 0;
            const int got = plan.size() > 1 && last.op == OP_LEVELS ? last.count : 0;
            CHECK(got == wt, "top-down tail %d, the rule gives %d", got, wt);
            if (got > 0) CHECK(last.arg == 1 && last.first == nd - wt, "the tail's launch");
        }
    }
    for (const PmlLaunch& r : plan) {
        if (bu && r.op == OP_LEVELS) CHECK(r.signal == (t.sched_cols <= 64 && !t.no_spin_wait), "bottom-up completion word");
        if (r.op != OP_LEVEL) continue;
        // the list: sorted by shape where the level launches walk the sorted lists (marginal fused sweeps, top-down)
        const bool sorted = r.list == L_BU_FUSED_SORTED || r.list == L_TD_FUSED_SORTED || r.list == L_REST_BU_SORTED || r.list == L_REST_TD_SORTED;
        const bool may_sort = r.list != L_BU_PLAIN && r.list != L_TD_PLAIN && r.list != L_TOP_BU && r.list != L_TOP_TD && branch != BU_FUSED_JOINT;
        CHECK(sorted == (may_sort && t.level_lists_sorted), "list %d with level_lists_sorted = %d", r.list, (int)t.level_lists_sorted);
        // the kind: VEC where some unit of the level has a stored node as child 0 or 1
        const std::vector<char>* vec = nullptr;
        const std::vector<int>* off = nullptr;
        if (r.list == L_BU_FUSED || r.list == L_BU_FUSED_SORTED) vec = &F.P.bu_level_vec_f, off = &f.bu_offsets_f;
        if (r.list == L_TOP_BU) vec = &B.top_bu_vec, off = &B.top_bu_offsets;
        if (r.list == L_REST_BU || r.list == L_REST_BU_SORTED) vec = &U.bu_level_vec_r, off = &U.bu_offsets_r;
        if (vec != nullptr) {
            const int l = level_of(*off, r);
            CHECK(l >= 0, "launch over entries %d + %d is no level", r.first, r.count);
            const bool joint = branch == BU_FUSED_JOINT;
            const int want = l < 0 ? -1 : (*vec)[l] ? (joint ? SW_BU_JOINT_FUSED : SW_BU_MARG_FUSED) : (joint ? SW_BU_JOINT_FUSED_NOVEC : SW_BU_MARG_FUSED_NOVEC);
            if (r.count > 0) CHECK(r.kind == want, "level %d kind %d, wanted %d", l, r.kind, want);
        }
        if (!bu) {
            CHECK(r.kind == (t.f81 ? SW_TD_FUSED : SW_TD), "top-down kind %d", r.kind);
            bool want = true;   // the hint comes from the prefix counts for the whole forest's fused list only
            const std::vector<int>& pre = F.P.td_cherry_prefix;
            if ((r.list == L_TD_FUSED || r.list == L_TD_FUSED_SORTED) && !pre.empty() && (size_t)(r.first + r.count) < pre.size())
                want = pre[r.first + r.count] != pre[r.first];
            CHECK(r.cherries == want, "staging hint %d of entries %d + %d", (int)r.cherries, r.first, r.count);
        }
    }
}

// ---- what a plan leaves behind for the host (pml_plan_outcome): the completion word's count, the cherry-fused joint branch
static PmlSweepOutcome check_outcome(const std::vector<PmlLaunch>& plan, bool joint_bottom_up) {
    const PmlSweepOutcome o = pml_plan_outcome(plan);
    int n_signal = 0;
    for (const PmlLaunch& r : plan) n_signal += r.signal ? 1 : 0;
    CHECK(o.n_signals == n_signal, "outcome counts %d signalling launches, the plan holds %d", o.n_signals, n_signal);
    CHECK(o.final_signals == (n_signal > 0 && plan.back().signal), "outcome: final_signals %d with %d signal records", (int)o.final_signals, n_signal);
    const bool fused_joint = !plan.empty() && plan.front().branch == BU_FUSED_JOINT;
    CHECK(o.fused_joint == fused_joint, "outcome: fused_joint %d for a plan of branch %d", (int)o.fused_joint, plan.empty() ? -1 : plan.front().branch);
    CHECK(!o.fused_joint || joint_bottom_up, "outcome: fused_joint for a plan that is no joint bottom-up sweep");
    CHECK(!o.has_params, "outcome: a plan holds no copy of the parameter block");
    return o;
}

static void run_case(const Planned& F, const PmlSweepTraits& t, const char* what) {
    long long got[5], want[5];
    PmlSweepOutcome marginal_sweep;
    for (int marginal = 0; marginal < 2; ++marginal) {
        g_case = std::string(what) + (marginal ? " bottom-up marginal" : " bottom-up joint");
        const std::vector<PmlLaunch> plan = pml_plan_bottom_up(F.f, F.S, t, marginal != 0);
        const int b = plan.front().branch;
        check_plan(F, plan, 0, b <= BU_FUSED_JOINT, got);
        check_rules(F, plan, t);
        expected_counts(F, plan, t, want);
        for (int i = 0; i < 5; ++i) CHECK(got[i] == want[i], "bracket %d: %lld records, the sweep counted %lld launches", i, got[i], want[i]);
        const PmlSweepOutcome o = check_outcome(plan, !marginal);
        if (marginal) marginal_sweep = o;
    }
    for (int wants = 0; wants < 2; ++wants) {
        g_case = std::string(what) + " top-down";
        const std::vector<PmlLaunch> plan = pml_plan_top_down(F.f, F.S, t, wants != 0);
        check_plan(F, plan, 1, t.f81, got);
        check_rules(F, plan, t);
        expected_counts(F, plan, t, want);
        for (int i = 0; i < 5; ++i) CHECK(got[i] == want[i], "bracket %d: %lld records, the sweep counted %lld launches", i, got[i], want[i]);
        bool signals = false;
        for (const PmlLaunch& r : plan) signals = signals || r.signal;
        CHECK(!signals || (wants && t.C <= 64 && !t.no_spin_wait), "a top-down launch signals unasked");
        // a marginal pass: the bottom-up sweep, then this one
        const PmlSweepOutcome td = check_outcome(plan, false);
        PmlSweepOutcome pass = marginal_sweep;
        pass.then(td);
        CHECK(pass.n_signals == marginal_sweep.n_signals + td.n_signals && pass.final_signals == td.final_signals && !pass.fused_joint,
              "the outcome of a pass: %d signals, final %d, fused_joint %d", pass.n_signals, (int)pass.final_signals, (int)pass.fused_joint);
    }
    g_case = std::string(what) + " back-trace";
    int head = -1;
    const std::vector<PmlLaunch> plan = pml_plan_backtrace(F.f, F.S, t, &head);
    if (F.nd() > 1) check_plan(F, plan, 2, false, got);
    check_outcome(plan, false);
    CHECK(head >= 0, "no head");
}

static void run_forest(const char* name, const Tree& T) {
    Planned F;
    F.t = {(int)T.parent.size(), T.n_roots, (int)T.bu_offsets.size() - 1, (int)T.td_offsets.size() - 1, T.parent.data(),
           T.first_child.data(), T.n_children.data(), T.bu_offsets.data(), T.bu_order.data(), T.td_offsets.data(),
           T.td_parent_offsets.data(), T.td_parents.data(), T.post_rank.data(), T.dist.data()};
    g_case = name;
    const std::string bad = pml_check_tree(F.t);
    CHECK(bad.empty(), "%s", bad.c_str());
    if (!bad.empty()) return;
    PmlTune tune;
    F.f = pml_plan_forest(F.t, tune, true, F.num);
    F.P = pml_plan_tree(F.f, F.t, tune);
    F.H = pml_plan_thin_ends(F.f, tune, 4096);
    F.S = {&F.P.blocks.s, &F.H.thin, &F.H.deep, &F.P.sup.s, &F.P.eig.s, &F.P.bt.s, &F.P.bu_level_vec_f, &F.P.bu_level_vec,
           &F.P.td_cherry_prefix};
    PmlSweepTraits base = {};
    base.fuse = true;
    base.n_roots = T.n_roots;
    base.n_cherries = (int)F.P.cherries.size();
    base.waves = 4;
    base.eig_nb = 1;
    struct Shape { int k, Gf, Gt; bool wide_lanes; } shapes[] = {{4, 2, 2, false}, {12, 4, 4, false}, {64, 16, 8, true}};
    const int cols[][2] = {{1, 1}, {32, 32}, {128, 128}, {128, 32}};
    char what[256];
    for (const Shape& s : shapes)
        for (const auto& c : cols)
            for (int sched = 0; sched < 5; ++sched)
                for (int variant = 0; variant < 4; ++variant) {
                    PmlSweepTraits t = base;
                    t.f81 = true;
                    t.k = s.k; t.W = 1; t.Gf = s.Gf; t.Gt = s.Gt; t.bu_wide_lanes = s.wide_lanes;
                    t.level_lists_sorted = s.Gf >= 4;
                    t.C = c[0]; t.sched_cols = c[1];
                    t.single_launch = sched == 1;
                    t.blocks = sched == 2 && F.P.blocks.s.ok;
                    t.super = sched == 3 && F.P.sup.s.ok && s.Gf >= 8;
                    t.thin = sched == 4 && F.H.thin.ok;
                    t.deep = sched == 4 && F.H.deep.ok;
                    t.narrow_units = variant == 1 ? 64 : 0;
                    t.no_td_tail = variant == 2;
                    t.no_spin_wait = variant == 3;
                    t.has_init = variant == 2;
                    snprintf(what, sizeof(what), "%s F81 k=%d C=%d/%d schedule %d variant %d", name, s.k, c[0], c[1], sched, variant);
                    run_case(F, t, what);
                }
    // the other model families: eigen joint on the vector units / two-GEMM (with and without tiers) / fused, HKY, matrix, wide F81
    for (int path = 0; path < 7; ++path)
        for (const auto& c : cols) {
            PmlSweepTraits t = base;
            t.k = path == 6 ? 300 : 20; t.W = path == 6 ? 5 : 1; t.Gf = t.Gt = path == 6 ? 64 : 8;
            t.C = t.sched_cols = c[0];
            t.eigen_joint_valu = path <= 2;
            t.eigen_gemm = path == 0 || path == 1;
            t.no_eigg_tiers = path == 1;
            t.eigen_fused = path == 2 || path == 3;
            t.eig_nb = 4;
            t.hky_fused = path == 4;
            t.f81 = t.wide_states = path == 6;
            snprintf(what, sizeof(what), "%s path %d C=%d", name, path, c[0]);
            run_case(F, t, what);
        }
}

int main() {
    const std::function<std::vector<int>(int)> even = split_even, comb = split_comb, rnd = split_random, poly = split_poly;
    run_forest("balanced 2^10", grow({1 << 10}, even));
    run_forest("balanced 2^14", grow({1 << 14}, even));
    run_forest("balanced 2^17", grow({1 << 17}, even));
    run_forest("caterpillar 10000", grow({10001}, comb));
    run_forest("random 3000", grow({3000}, rnd));
    run_forest("random 40000", grow({40000}, rnd));
    run_forest("random 262144", grow({262144}, rnd));
    run_forest("polytomies 20000", grow({20000}, poly));
    run_forest("star 5000", grow({5000}, [](int n) { return std::vector<int>(n, 1); }));
    {
        std::vector<int> budgets;
        for (int i = 0; i < 200; ++i) budgets.push_back(2 + (int)(g_rng() % 30));
        run_forest("forest of 200", grow(budgets, rnd));
    }
    g_case = "all inputs";
    for (int op = 0; op < OP_COUNT; ++op) CHECK(g_ops.count(op), "op %d is never planned", op);
    for (int b = 0; b < PML_BRANCH_COUNT; ++b) CHECK(g_branches.count(b), "schedule branch %d is never reached", b);
    if (g_failures) {
        printf("%d failures\n", g_failures);
        return 1;
    }
    printf("OK: %zu ops, %zu branches\n", g_ops.size(), g_branches.size());
    return 0;
}
