// Host-only check of the chained bottom-up launch's planning (pastml_amd/csrc/pml_schedule.h: PmlSuperSchedule::bu_chain_level,
// PmlSweepTraits::bu_chain): where pml_plan_tree finds a chain, and what pml_plan_bottom_up makes of it -- every stored node's
// vector (with pi . v and the exponent) written by exactly one record, no record reading one before the record that writes it,
// the chained stacked units' grandchildren all two-level nodes, and nothing else changed in the plan.
// Built and run by tests/test_bu_chain_plan_host.py; prints FAIL lines and exits 1, or one OK line.
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

// ---- vectors of stored nodes: what a record of a BU_SUPER plan reads from memory and what it writes
struct Vecs {
    std::vector<int> reads, writes;
    bool orders_itself = false;   // the launch orders vectors it writes and reads itself (a barrier between levels, a wave's LDS)
};
static Vecs vecs_of(const Planned& F, const PmlLaunch& r) {
    const PmlForest& f = F.f;
    const PmlSuperSchedule& U = F.P.sup.s;
    Vecs R;
    auto stored = [&](int n) { return f.kind[n] == PML_KIND_STORED; };
    auto unit = [&](int n) {   // a level unit: its stored children in (cherries and tips are rebuilt from the masks), the node out
        for (int j = 0; j < f.n_children[n]; ++j)
            if (stored(f.first_child[n] + j)) R.reads.push_back(f.first_child[n] + j);
        R.writes.push_back(n);
    };
    auto stacked = [&](int level) {   // a stacked unit: four grandchildren in, the two children and the node out
        for (int i = U.stack_bu_offsets[level]; i < U.stack_bu_offsets[level + 1]; ++i) {
            const PmlUnit& s = F.P.sup.stack_bu[i];
            CHECK(f.n_children[s.n] == 2 && s.fc == f.first_child[s.n], "stacked unit %d: node %d", i, s.n);
            for (int j = 0; j < 2; ++j) {
                const int ch = s.fc + j;
                CHECK(stored(ch) && f.n_children[ch] == 2 && s.cfc[j] == f.first_child[ch], "stacked unit %d: child %d", i, ch);
                R.reads.push_back(s.cfc[j]);
                R.reads.push_back(s.cfc[j] + 1);
                R.writes.push_back(ch);
            }
            R.writes.push_back(s.n);
        }
    };
    switch (r.op) {
        case OP_RESET_ERR:
        case OP_PREP: break;
        case OP_LOGLIK:
            for (int n = 0; n < f.n_roots; ++n)
                if (stored(n)) R.reads.push_back(n);
            break;
        case OP_LEVELS:   // the levels next to the roots, a barrier in between
            R.orders_itself = true;
            for (int i = U.bu_offsets_r[r.first]; i < U.bu_offsets_r[r.first + r.count]; ++i) unit(F.P.sup.bu_units_r[i].n);
            break;
        case OP_LEVEL:
            for (int i = r.first; i < r.first + r.count; ++i)
                unit((r.list == L_REST_BU_SORTED ? F.P.sup.bu_units_rs : F.P.sup.bu_units_r)[i].n);
            break;
        case OP_STACK: stacked(r.first); break;
        case OP_SUPER: {
            std::vector<char> two_level(f.N, 0);
            for (int i = 0; i < U.n; ++i) {   // a two-level unit reads tips only
                const PmlUnit& u = F.P.sup.units[i];
                two_level[u.n] = 1;
                R.writes.push_back(u.fc);
                R.writes.push_back(u.fc + 1);
                R.writes.push_back(u.n);
            }
            if (r.arg > 0) {
                // what makes the front of the sweep safe for them: all they read is what this launch writes
                for (int i = U.stack_bu_offsets[r.arg - 1]; i < U.stack_bu_offsets[r.arg]; ++i)
                    for (int q = 0; q < 4; ++q) {
                        const int g = F.P.sup.stack_bu[i].cfc[q >> 1] + (q & 1);
                        CHECK(two_level[g], "chained stacked unit %d reads node %d, which is no two-level node", i, g);
                    }
                R.orders_itself = true;
                stacked(r.arg - 1);
            }
            break;
        }
        default: CHECK(false, "op %d in a bottom-up plan of the two-level schedule", r.op);
    }
    return R;
}

static void check_vecs(const Planned& F, const std::vector<PmlLaunch>& plan) {
    const PmlForest& f = F.f;
    std::vector<int> written(f.N, -1);
    for (size_t idx = 0; idx < plan.size(); ++idx) {
        const Vecs R = vecs_of(F, plan[idx]);
        for (int n : R.writes) {
            CHECK(written[n] < 0, "vector of node %d written by records %d and %zu", n, written[n], idx);
            written[n] = (int)idx;
        }
        for (int n : R.reads)
            CHECK(written[n] >= 0 && (written[n] < (int)idx || R.orders_itself),
                  "record %zu (op %d) reads the vector of node %d before a record has written it", idx, plan[idx].op, n);
    }
    for (int n = 0; n < f.N; ++n)
        if (f.kind[n] == PML_KIND_STORED) CHECK(written[n] >= 0, "vector of stored node %d is written by no record", n);
}

static bool same(const PmlLaunch& a, const PmlLaunch& b) {
    return a.op == b.op && a.list == b.list && a.kind == b.kind && a.bracket == b.bracket && a.branch == b.branch && a.signal == b.signal &&
           a.cherries == b.cherries && a.first == b.first && a.count == b.count && a.arg == b.arg;
}

// want: the chained level the forest must get; stack_min: PASTML_HIP_STACK_MIN for the planner, 0 = its default
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
    CHECK(U.bu_chain_level == want, "chained level %d, wanted %d (%d two-level, %d stacked units)", U.bu_chain_level, want, U.n, U.n_stack);
    CHECK(U.ok, "no two-level schedule");
    if (!U.ok) return;
    if (U.bu_chain_level >= 0) {
        // the conditions, restated on the lists the kernel walks
        const int a = U.stack_bu_offsets[U.bu_chain_level], cnt = U.stack_bu_offsets[U.bu_chain_level + 1] - a;
        CHECK(cnt > 0 && 4 * cnt == U.n, "%d stacked units of the level for %d two-level units", cnt, U.n);
        CHECK(a == 0, "%d stacked units below the chained level", a);
        for (int m = 0; m < cnt && 4 * cnt == U.n; ++m) {
            const PmlUnit& s = F.P.sup.stack_bu[a + m];
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
        for (int sorted = 0; sorted < 2; ++sorted) {
            PmlSweepTraits t = base;
            t.C = t.sched_cols = C;
            t.level_lists_sorted = sorted != 0 && !F.P.sup.bu_units_rs.empty();
            snprintf(what, sizeof(what), "%s C=%d sorted=%d", name, C, (int)t.level_lists_sorted);
            g_case = what;
            const std::vector<PmlLaunch> off = pml_plan_bottom_up(F.f, F.S, t, true);
            t.bu_chain = true;
            const std::vector<PmlLaunch> on = pml_plan_bottom_up(F.f, F.S, t, true);
            // the joint sweep does not know the trait
            const std::vector<PmlLaunch> joint_on = pml_plan_bottom_up(F.f, F.S, t, false);
            t.bu_chain = false;
            const std::vector<PmlLaunch> joint_off = pml_plan_bottom_up(F.f, F.S, t, false);
            CHECK(joint_on.size() == joint_off.size() && std::equal(joint_on.begin(), joint_on.end(), joint_off.begin(), same),
                  "the joint sweep's plan changes with the trait");
            // the switch off: the two-level record opens the sweep's launches in bracket 4 on its own, a stacked record per
            // stacked level
            int n_stack = 0, levels = 0, n_super = 0;
            for (size_t l = 0; l + 1 < U.stack_bu_offsets.size(); ++l) levels += U.stack_bu_offsets[l + 1] > U.stack_bu_offsets[l];
            for (const PmlLaunch& r : off) {
                n_stack += r.op == OP_STACK;
                CHECK(r.branch == BU_SUPER, "branch %d", r.branch);
                if (r.op == OP_SUPER) {
                    ++n_super;
                    CHECK(r.arg == 0 && r.bracket == 4, "the two-level record of the unchained plan");
                }
            }
            CHECK(n_super == (U.n > 0) && (U.n == 0 || (off.size() > 2 && off[2].op == OP_SUPER)), "the two-level record opens the unchained plan's launches");
            CHECK(n_stack == levels, "%d stacked records for %d stacked levels", n_stack, levels);
            check_vecs(F, off);
            check_vecs(F, on);
            if (U.bu_chain_level < 0) {
                CHECK(on.size() == off.size() && std::equal(on.begin(), on.end(), off.begin(), same), "no chain, but the plans differ");
                continue;
            }
            // the chained plan: the unchained one without the stacked record of the level, the level in the opening record's arg
            std::vector<PmlLaunch> expect;
            int dropped = 0;
            for (const PmlLaunch& r : off) {
                if (r.op == OP_STACK && r.first == U.bu_chain_level) {
                    ++dropped;
                    continue;
                }
                expect.push_back(r);
                if (r.op == OP_SUPER) expect.back().arg = U.bu_chain_level + 1;
            }
            CHECK(dropped == 1, "%d stacked records of level %d in the unchained plan", dropped, U.bu_chain_level);
            CHECK(on.size() == expect.size() && std::equal(on.begin(), on.end(), expect.begin(), same),
                  "the chained plan is not the unchained one less the stacked record (%zu records against %zu)", on.size(), expect.size());
            CHECK(on.size() > 2 && on[2].op == OP_SUPER && on[2].bracket == 4 && on[2].arg == U.bu_chain_level + 1, "the chained record");
        }
}

int main() {
    const std::function<std::vector<int>(int)> even = split_even, rnd = split_random;
    // fused heights: cherries 0 (no level of their own), their parents level 0, two-level nodes level 1, stacked nodes level 3
    run_forest("balanced 2^13", grow({1 << 13}, even), 3, 64);
    run_forest("balanced 2^15", grow({1 << 15}, even), 3, 0);
    run_forest("balanced 2^17", grow({1 << 17}, even), 3, 0);
    run_forest("four balanced 2^13", grow({1 << 13, 1 << 13, 1 << 13, 1 << 13}, even), 3, 0);
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
