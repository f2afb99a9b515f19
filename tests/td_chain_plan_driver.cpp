// Host-only check of the chained top-down launch's planning (pastml_amd/csrc/pml_schedule.h: PmlSuperSchedule::chain_depth,
// PmlSweepTraits::td_chain): where pml_plan_tree finds a chain, and what pml_plan_top_down makes of it -- every stored node's row
// written by exactly one record, no record reading a row before the record that writes it, and nothing else changed in the plan.
// Built and run by tests/test_td_chain_plan_host.py; prints FAIL lines and exits 1, or one OK line.
#include "../pastml_amd/csrc/pml_schedule.h"

#include <algorithm>
#include <cstdio>
#include <functional>
#include <random>

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

static std::mt19937 g_rng(4711);
static std::vector<int> split_even(int n) { return {n - n / 2, n / 2}; }
static std::vector<int> split_random(int n) {
    const int a = 1 + (int)(g_rng() % (unsigned)(n - 1));
    return {a, n - a};
}

struct Planned {
    PmlForest f;
    PmlNumbering num;
    PmlTreeArrays t;
    PmlTreePlan P;
    PmlThinPlan H;
    PmlSchedules S;
};

// ---- rows of stored nodes: what a record of a TD_SUPER plan reads from memory and what it writes
struct Rows {
    std::vector<int> reads, writes;
    bool orders_itself = false;   // the launch orders rows it writes and reads itself (a barrier between levels, a wave's LDS)
};
static Rows rows_of(const Planned& F, const PmlLaunch& r) {
    const PmlForest& f = F.f;
    const PmlSuperSchedule& U = F.P.sup.s;
    Rows R;
    auto stored = [&](int n) { return f.kind[n] == PML_KIND_STORED; };
    auto children = [&](int n) {
        for (int j = 0; j < f.n_children[n]; ++j)
            if (stored(f.first_child[n] + j)) R.writes.push_back(f.first_child[n] + j);
    };
    auto stacked = [&](int depth) {   // a stacked unit: the node's row in, its children's and grandchildren's rows out
        for (int i = U.stack_td_offsets[depth]; i < U.stack_td_offsets[depth + 1]; ++i) {
            const int n = F.P.sup.stack_td[i].n;
            R.reads.push_back(n);
            children(n);
            for (int j = 0; j < f.n_children[n]; ++j) children(f.first_child[n] + j);
        }
    };
    switch (r.op) {
        case OP_ROOTS:
            for (int n = 0; n < f.n_roots; ++n)
                if (stored(n)) R.writes.push_back(n);
            break;
        case OP_LEVELS:   // the roots and the levels below them, a barrier in between
            R.orders_itself = true;
            for (int n = 0; n < f.n_roots; ++n)
                if (stored(n)) R.writes.push_back(n);
            for (int i = U.td_offsets_r[r.first]; i < U.td_offsets_r[r.first + r.count]; ++i) {
                R.reads.push_back(F.P.sup.td_units_r[i].n);
                children(F.P.sup.td_units_r[i].n);
            }
            break;
        case OP_LEVEL:
            for (int i = r.first; i < r.first + r.count; ++i) {
                const int n = (r.list == L_REST_TD_SORTED ? F.P.sup.td_units_rs : F.P.sup.td_units_r)[i].n;
                R.reads.push_back(n);
                children(n);
            }
            break;
        case OP_STACK: stacked(r.first); break;
        case OP_SUPER:
            if (r.arg > 0) {
                R.orders_itself = true;
                stacked(r.arg - 1);
            }
            for (int i = 0; i < U.n; ++i) {
                R.reads.push_back(F.P.sup.units[i].n);
                children(F.P.sup.units[i].n);
            }
            break;
        default: CHECK(false, "op %d in a top-down plan of the two-level schedule", r.op);
    }
    return R;
}

static void check_rows(const Planned& F, const std::vector<PmlLaunch>& plan) {
    const PmlForest& f = F.f;
    std::vector<int> written(f.N, -1);
    for (size_t idx = 0; idx < plan.size(); ++idx) {
        const Rows R = rows_of(F, plan[idx]);
        for (int n : R.writes) {
            CHECK(written[n] < 0, "row of node %d written by records %d and %zu", n, written[n], idx);
            written[n] = (int)idx;
        }
        for (int n : R.reads)
            CHECK(written[n] >= 0 && (written[n] < (int)idx || R.orders_itself),
                  "record %zu (op %d) reads the row of node %d before a record has written it", idx, plan[idx].op, n);
    }
    for (int n = 0; n < f.N; ++n)
        if (f.kind[n] == PML_KIND_STORED) CHECK(written[n] >= 0, "row of stored node %d is written by no record", n);
}

static bool same(const PmlLaunch& a, const PmlLaunch& b) {
    return a.op == b.op && a.list == b.list && a.kind == b.kind && a.bracket == b.bracket && a.branch == b.branch && a.signal == b.signal &&
           a.cherries == b.cherries && a.first == b.first && a.count == b.count && a.arg == b.arg;
}

// want: the chain depth the forest must get; stack_min: PASTML_HIP_STACK_MIN for the planner, 0 = its default
static void run_forest(const char* name, const Tree& T, int want, int stack_min) {
    Planned F;
    F.t = {(int)T.parent.size(), T.n_roots, (int)T.bu_offsets.size() - 1, (int)T.td_offsets.size() - 1, T.parent.data(),
           T.first_child.data(), T.n_children.data(), T.bu_offsets.data(), T.bu_order.data(), T.td_offsets.data(),
           T.td_parent_offsets.data(), T.td_parents.data(), T.post_rank.data(), T.dist.data()};
    g_case = name;
    const std::string bad = pml_check_tree(F.t);
    CHECK(bad.empty(), "%s", bad.c_str());
    if (!bad.empty()) return;
    PmlTune tune;
    for (int i = 0; i < T_COUNT; ++i) tune.has[i] = false;   // (whatever the environment says)
    if (stack_min > 0) {
        tune.has[T_STACK_MIN] = true;
        tune.val[T_STACK_MIN] = stack_min;
    }
    F.f = pml_plan_forest(F.t, tune, true, F.num);
    F.P = pml_plan_tree(F.f, F.t, tune);
    F.H = pml_plan_thin_ends(F.f, tune, 4096);
    F.S = {&F.P.blocks.s, &F.H.thin, &F.H.deep, &F.P.sup.s, &F.P.eig.s, &F.P.bt.s, &F.P.bu_level_vec_f, &F.P.bu_level_vec,
           &F.P.td_cherry_prefix};
    const PmlSuperSchedule& U = F.P.sup.s;
    CHECK(U.chain_depth == want, "chain depth %d, wanted %d (%d two-level, %d stacked units)", U.chain_depth, want, U.n, U.n_stack);
    CHECK(U.ok, "no two-level schedule");
    if (!U.ok) return;
    if (U.chain_depth >= 0) {
        // the conditions, restated on the lists the kernel walks
        const int a = U.stack_td_offsets[U.chain_depth], cnt = U.stack_td_offsets[U.chain_depth + 1] - a;
        CHECK(cnt > 0 && 4 * cnt == U.n, "%d stacked units of the depth for %d two-level units", cnt, U.n);
        for (size_t l = U.chain_depth + 1; l + 1 < U.stack_td_offsets.size(); ++l)
            CHECK(U.stack_td_offsets[l + 1] == U.stack_td_offsets[l], "stacked units below the chained depth, at %zu", l);
        for (int m = 0; m < cnt && 4 * cnt == U.n; ++m) {
            const PmlUnit& s = F.P.sup.stack_td[a + m];
            for (int q = 0; q < 4; ++q)
                CHECK(F.P.sup.units[4 * m + q].n == s.cfc[q >> 1] + (q & 1), "two-level unit %d is node %d, stacked unit %d has grandchild %d there",
                      4 * m + q, F.P.sup.units[4 * m + q].n, m, s.cfc[q >> 1] + (q & 1));
        }
    }
    PmlSweepTraits base = {};
    base.f81 = base.fuse = base.super = true;
    base.k = 64; base.W = 1; base.Gf = 16; base.Gt = 8; base.bu_wide_lanes = true;
    base.n_roots = T.n_roots;
    base.n_cherries = (int)F.P.cherries.size();
    base.waves = 4;
    base.eig_nb = 1;
    const int cols[] = {1, 16, 40, 128};
    char what[256];
    for (int C : cols)
        for (int sorted = 0; sorted < 2; ++sorted)
            for (int wants = 0; wants < 2; ++wants) {
                PmlSweepTraits t = base;
                t.C = t.sched_cols = C;
                t.level_lists_sorted = sorted != 0 && !F.P.sup.td_units_rs.empty();
                snprintf(what, sizeof(what), "%s C=%d sorted=%d signal=%d", name, C, (int)t.level_lists_sorted, wants);
                g_case = what;
                const std::vector<PmlLaunch> off = pml_plan_top_down(F.f, F.S, t, wants != 0);
                t.td_chain = true;
                const std::vector<PmlLaunch> on = pml_plan_top_down(F.f, F.S, t, wants != 0);
                // the switch off: a stacked launch per stacked depth below the head, the two-level launch last and on its own
                int n_stack = 0, depths = 0;
                const int head = off.front().op == OP_LEVELS ? off.front().count : 0;
                for (size_t l = head; l + 1 < U.stack_td_offsets.size(); ++l) depths += U.stack_td_offsets[l + 1] > U.stack_td_offsets[l];
                for (const PmlLaunch& r : off) {
                    n_stack += r.op == OP_STACK;
                    CHECK(r.branch == TD_SUPER, "branch %d", r.branch);
                    if (r.op == OP_SUPER) CHECK(r.arg == 0 && r.bracket == 3 && &r == &off.back(), "the two-level record of the unchained plan");
                }
                CHECK(n_stack == depths, "%d stacked records for %d stacked depths", n_stack, depths);
                check_rows(F, off);
                check_rows(F, on);
                if (U.chain_depth < 0) {
                    CHECK(on.size() == off.size() && std::equal(on.begin(), on.end(), off.begin(), same), "no chain, but the plans differ");
                    continue;
                }
                // the chained plan: the unchained one without the stacked record of the depth, the depth in the last record's arg
                std::vector<PmlLaunch> expect;
                int dropped = 0;
                for (const PmlLaunch& r : off) {
                    if (r.op == OP_STACK && r.first == U.chain_depth) {
                        ++dropped;
                        continue;
                    }
                    expect.push_back(r);
                    if (r.op == OP_SUPER) expect.back().arg = U.chain_depth + 1;
                }
                CHECK(dropped == 1, "%d stacked records of depth %d in the unchained plan", dropped, U.chain_depth);
                CHECK(on.size() == expect.size() && std::equal(on.begin(), on.end(), expect.begin(), same),
                      "the chained plan is not the unchained one less the stacked record (%zu records against %zu)", on.size(), expect.size());
                CHECK(on.back().op == OP_SUPER && on.back().bracket == 3 && on.back().arg == U.chain_depth + 1, "the chained record");
            }
}

int main() {
    const std::function<std::vector<int>(int)> even = split_even, rnd = split_random;
    // tips at depth L, two-level nodes at L - 3, the stacked nodes right above them at L - 5
    run_forest("balanced 2^13", grow({1 << 13}, even), 8, 64);
    run_forest("balanced 2^15", grow({1 << 15}, even), 10, 0);
    run_forest("balanced 2^17", grow({1 << 17}, even), 12, 0);
    run_forest("four balanced 2^13", grow({1 << 13, 1 << 13, 1 << 13, 1 << 13}, even), 8, 0);
    run_forest("random 40000", grow({40000}, rnd), -1, 64);
    run_forest("random forest", grow({30000, 20000, 500}, rnd), -1, 64);
    run_forest("balanced 2^15 and 2^13", grow({1 << 15, 1 << 13}, even), -1, 0);
    run_forest("balanced 2^15 and 2^13, small stacked levels", grow({1 << 15, 1 << 13}, even), -1, 64);
    run_forest("balanced 2^15 less a tip pair", grow({(1 << 15) - 1}, even), -1, 0);
    run_forest("balanced 2^13 less a tip pair, small stacked levels", grow({(1 << 13) - 1}, even), -1, 64);
    if (g_failures) {
        printf("%d failures\n", g_failures);
        return 1;
    }
    printf("OK\n");
    return 0;
}
