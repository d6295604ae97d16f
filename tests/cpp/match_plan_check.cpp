// What the matcher kernels rely on in the pair plan of easysfm_amd/csrc/match_plan.cpp, checked on the CPU over seeded set sizes and
// pair lists (tests/test_match_plan.py builds this against match_plan.cpp alone), with the plain matcher's rules and the guided
// matcher's.  Each block names who reads the table and what is assumed without checking.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "match_plan.hpp"

using namespace esfm;

// the library's error text (ctx.cpp), kept here so that the messages can be compared
static std::string g_error;
void esfm::set_error(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
}

namespace {

int g_failed = 0;
std::string g_case;
#define REQUIRE(cond, ...)                                                                                     \
    do {                                                                                                       \
        if (!(cond)) {                                                                                         \
            if (g_failed++ < 40) { printf("FAIL [%s] %s:%d %s  ", g_case.c_str(), __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
            return;                                                                                            \
        }                                                                                                      \
    } while (0)

constexpr int64_t kSentinel = -0x5E5E5E5E5E5Ell;

std::vector<int32_t> offsets_of(const std::vector<int32_t> &sizes)
{
    std::vector<int32_t> off(sizes.size() + 1, 0);
    for (size_t s = 0; s < sizes.size(); ++s) off[s + 1] = off[s] + sizes[s];
    return off;
}

int64_t blocks(int64_t n, int b) { return (n + b - 1) / b; }

struct Rules { int query_block, query_block2; bool mirror; const PlanRules &r; };

// One plan, every table against its definition.
void check(const std::vector<int32_t> &sizes, const std::vector<int32_t> &pairs, const Rules &rules)
{
    const std::vector<int32_t> off = offsets_of(sizes);
    const int P = (int)(pairs.size() / 2), n_sets = (int)sizes.size();
    const size_t G = (size_t)P * (rules.mirror ? 2 : 1);
    std::vector<int64_t> out_offset(2 * (size_t)P + 2, kSentinel);
    PairPlan plan;
    const int rc = make_plan(off.data(), n_sets, pairs.data(), P, rules.query_block, rules.query_block2, rules.mirror, rules.r, out_offset.data(), &plan);
    REQUIRE(rc == ESFM_OK, "rc %d: %s", rc, g_error.c_str());
    REQUIRE(plan.tab.size() == G && plan.n_fwd == P && plan.total_rows == off[(size_t)n_sets], "sizes");

    // ---- the pair table (every kernel: rows [q_row0, q_row0 + nq) against rows [t_row0, t_row0 + nt); output slot out_off + q;
    // find_pair_by_block / find_pair_by_query search blk_off / out_off, which therefore must be the prefix sums) ----
    int64_t o = 0, b = 0, b2 = 0;
    int max_nt = 0;
    for (size_t g = 0; g < G; ++g) {
        const int p = (int)(g % (size_t)P);
        const bool rev = g >= (size_t)P;
        const int qs = pairs[2 * (size_t)p + (rev ? 1 : 0)], ts = pairs[2 * (size_t)p + (rev ? 0 : 1)];
        const PairDesc &d = plan.tab[g];
        REQUIRE(d.q_row0 == off[(size_t)qs] && d.nq == sizes[(size_t)qs] && d.t_row0 == off[(size_t)ts] && d.nt == sizes[(size_t)ts], "sets of entry %zu", g);
        REQUIRE(d.out_off == o, "out_off of entry %zu: %lld, prefix sum %lld", g, (long long)d.out_off, (long long)o);
        REQUIRE(d.blk_off == b, "blk_off of entry %zu", g);
        REQUIRE(d.blk_off2 == b2, "blk_off2 of entry %zu", g);
        if (!rev) REQUIRE(out_offset[(size_t)p] == o, "out_offset[%d]", p);
        o += d.nq;
        b += blocks(d.nq, rules.query_block);
        if (rules.query_block2 > 0) b2 += blocks(d.nq, rules.query_block2);
        max_nt = std::max(max_nt, (int)d.nt);
        if (g + 1 == (size_t)P) REQUIRE(plan.fwd_queries == o, "fwd_queries");
    }
    if (P == 0) REQUIRE(plan.fwd_queries == 0, "fwd_queries of an empty list");
    REQUIRE(plan.total_queries == o && plan.n_blocks == b && plan.n_blocks2 == b2 && plan.max_nt == max_nt, "totals");
    // the caller's array: P + 1 entries, the forward total last, nothing behind it -- of a mirrored plan too
    REQUIRE(out_offset[(size_t)P] == plan.fwd_queries, "out_offset[P]");
    for (size_t k = (size_t)P + 1; k < out_offset.size(); ++k) REQUIRE(out_offset[k] == kSentinel, "out_offset[%zu] was written", k);

    // ---- the mirrored half (cross_check_compact_kernel, guided_knn2_kernel: entry P + p is pair p with the roles swapped, its slots
    // behind the forward pairs') ----
    if (rules.mirror) {
        for (int p = 0; p < P; ++p) {
            const PairDesc &f = plan.tab[(size_t)p], &m = plan.tab[(size_t)P + (size_t)p];
            REQUIRE(m.q_row0 == f.t_row0 && m.nq == f.nt && m.t_row0 == f.q_row0 && m.nt == f.nq, "mirror of pair %d", p);
            REQUIRE(m.out_off >= plan.fwd_queries, "mirror %d writes into the forward slots", p);
        }
        if (P) REQUIRE(plan.tab[(size_t)P].out_off == plan.fwd_queries, "the mirrors continue the forward total");
    }

    // ---- the front pass's block table (l2_knn_bf16x1_kernel, hamming_fp4_kernel: workgroup b works on pair blk_pair[b], block
    // b - blk_off2 of it) and the pair order of l2_finish_kernel ----
    if (rules.query_block2 > 0) {
        REQUIRE(plan.blk_pair.size() == (size_t)b2, "blk_pair size");
        for (size_t g = 0; g < G; ++g) {
            const int64_t lo = plan.tab[g].blk_off2, hi = g + 1 < G ? plan.tab[g + 1].blk_off2 : b2;
            for (int64_t k = lo; k < hi; ++k) REQUIRE(plan.blk_pair[(size_t)k] == (int32_t)g, "blk_pair[%lld] is not %zu", (long long)k, g);
        }
        REQUIRE(plan.by_train.size() == G, "by_train size");
        std::vector<char> seen(G, 0);
        for (size_t k = 0; k < G; ++k) {
            const int32_t g = plan.by_train[k];
            REQUIRE(g >= 0 && (size_t)g < G && !seen[(size_t)g], "by_train is not a permutation at %zu", k);
            seen[(size_t)g] = 1;
            if (k) {
                const int32_t h = plan.by_train[k - 1];
                REQUIRE(plan.tab[(size_t)h].t_row0 < plan.tab[(size_t)g].t_row0 || (plan.tab[(size_t)h].t_row0 == plan.tab[(size_t)g].t_row0 && h < g),
                        "by_train is not the stable sort by t_row0 at %zu", k);
            }
        }
    } else {
        REQUIRE(plan.blk_pair.empty() && plan.by_train.empty() && plan.n_blocks2 == 0, "tables nobody asked for");
    }
}

void run(const char *name, const std::vector<int32_t> &sizes, const std::vector<int32_t> &pairs)
{
    for (int qb : {128, 256})
        for (int mirror = 0; mirror < 2; ++mirror) {
            g_case = std::string(name) + " plain qb " + std::to_string(qb) + (mirror ? " mirrored" : "");
            check(sizes, pairs, Rules{qb, 512, mirror != 0, kPlainPlanRules});
        }
    for (int mirror = 0; mirror < 2; ++mirror) {
        g_case = std::string(name) + " guided" + (mirror ? " mirrored" : "");
        check(sizes, pairs, Rules{256, 0, mirror != 0, kGuidedPlanRules});
    }
}

// a refused call: code and text
void refused(const char *what, int rc, int want_rc, const char *want_msg)
{
    g_case = what;
    REQUIRE(rc == want_rc, "rc %d, expected %d", rc, want_rc);
    REQUIRE(g_error == want_msg, "message \"%s\", expected \"%s\"", g_error.c_str(), want_msg);
}
void accepted(const char *what, int rc)
{
    g_case = what;
    REQUIRE(rc == ESFM_OK, "rc %d: %s", rc, g_error.c_str());
}

int plan_rc(const std::vector<int32_t> &sizes, const std::vector<int32_t> &pairs, const Rules &rules)
{
    const std::vector<int32_t> off = offsets_of(sizes);
    std::vector<int64_t> out(pairs.size() / 2 + 1);
    PairPlan plan;
    g_error.clear();
    return make_plan(off.data(), (int)sizes.size(), pairs.data(), (int)(pairs.size() / 2), rules.query_block, rules.query_block2, rules.mirror, rules.r, out.data(), &plan);
}

void limits()
{
    const int M21 = 1 << 21, M23 = 1 << 23;
    const Rules plain{256, 512, false, kPlainPlanRules}, plain_m{256, 512, true, kPlainPlanRules};
    const Rules guided{256, 0, false, kGuidedPlanRules}, guided_m{256, 0, true, kGuidedPlanRules};
    // sets {0: 2^21 - 1, 1: 2^21, 2: 2^23 - 1, 3: 2^23, 4: 5}; a pair is (query set, train set)
    const std::vector<int32_t> sizes = {M21 - 1, M21, M23 - 1, M23, 5};
    const char *train = "make_plan: train sets are limited to 2^21-1 rows", *query = "make_plan: query sets are limited to 2^23-1 rows";
    const char *both = "make_plan: sets are limited to 2^21-1 rows";
    accepted("plain: train 2^21 - 1", plan_rc(sizes, {4, 0}, plain));
    refused("plain: train 2^21", plan_rc(sizes, {4, 1}, plain), ESFM_ERR_INVALID_ARG, train);
    accepted("plain: query 2^23 - 1", plan_rc(sizes, {2, 4}, plain));
    refused("plain: query 2^23", plan_rc(sizes, {3, 4}, plain), ESFM_ERR_INVALID_ARG, query);
    refused("plain: both too large, the train set is named", plan_rc(sizes, {3, 1}, plain), ESFM_ERR_INVALID_ARG, train);
    accepted("plain mirrored: both 2^21 - 1", plan_rc(sizes, {0, 0}, plain_m));
    refused("plain mirrored: query 2^21 is the mirror's train set", plan_rc(sizes, {1, 4}, plain_m), ESFM_ERR_INVALID_ARG, train);
    accepted("guided: both 2^21 - 1", plan_rc(sizes, {0, 0}, guided_m));
    refused("guided: train 2^21", plan_rc(sizes, {4, 1}, guided), ESFM_ERR_INVALID_ARG, both);
    refused("guided: query 2^21", plan_rc(sizes, {1, 4}, guided), ESFM_ERR_INVALID_ARG, both);
    refused("guided: query 2^23 - 1", plan_rc(sizes, {2, 4}, guided), ESFM_ERR_INVALID_ARG, both);

    // the argument checks, in their order
    const int32_t off_ok[3] = {0, 4, 9}, off_first[3] = {1, 4, 9}, off_down[3] = {0, 4, 3}, pr[2] = {1, 0}, pr_bad[2] = {1, 2};
    int64_t out[2];
    PairPlan plan;
    g_error.clear();
    refused("no offsets", make_plan(nullptr, 2, pr, 1, 256, 512, false, kPlainPlanRules, out, &plan), ESFM_ERR_INVALID_ARG, "make_plan: set_row_offset/n_sets");
    refused("no sets", make_plan(off_ok, 0, pr, 1, 256, 512, false, kPlainPlanRules, out, &plan), ESFM_ERR_INVALID_ARG, "make_plan: set_row_offset/n_sets");
    refused("plain: no pairs", make_plan(off_ok, 2, nullptr, 1, 256, 512, false, kPlainPlanRules, out, &plan), ESFM_ERR_INVALID_ARG, "make_plan: pairs/n_pairs");
    refused("plain: negative n_pairs", make_plan(off_ok, 2, pr, -1, 256, 512, false, kPlainPlanRules, out, &plan), ESFM_ERR_INVALID_ARG, "make_plan: pairs/n_pairs");
    refused("guided: no pairs", make_plan(off_ok, 2, nullptr, 1, 256, 0, false, kGuidedPlanRules, out, &plan), ESFM_ERR_INVALID_ARG, "make_plan: pairs/n_pairs");
    refused("first offset", make_plan(off_first, 2, pr, 1, 256, 512, false, kPlainPlanRules, out, &plan), ESFM_ERR_INVALID_ARG, "make_plan: set_row_offset[0] must be 0");
    refused("decreasing offsets", make_plan(off_down, 2, pr, 1, 256, 512, false, kPlainPlanRules, out, &plan), ESFM_ERR_INVALID_ARG, "make_plan: set_row_offset must be non-decreasing");
    refused("set out of range", make_plan(off_ok, 2, pr_bad, 1, 256, 512, false, kPlainPlanRules, out, &plan), ESFM_ERR_INVALID_ARG, "make_plan: pair refers to a set out of range");
    {
        PairPlan none;
        accepted("n_pairs == 0 without a pair list", make_plan(off_ok, 2, nullptr, 0, 256, 512, true, kPlainPlanRules, out, &none));
        g_case = "n_pairs == 0";
        REQUIRE(out[0] == 0 && none.tab.empty() && none.n_blocks == 0 && none.total_queries == 0 && none.total_rows == 9, "empty plan");
    }
    accepted("out_offset may be NULL", make_plan(off_ok, 2, pr, 1, 256, 512, false, kPlainPlanRules, nullptr, &plan));

    // metric / width / context, and the row size
    const esfm_ctx *ctx = reinterpret_cast<const esfm_ctx *>(&plan);      // (only compared with NULL)
    refused("no context", check_metric_width(nullptr, ESFM_L2_F32, 64, "w"), ESFM_ERR_INVALID_ARG, "ctx is NULL");
    refused("metric", check_metric_width(ctx, (esfm_metric)7, 64, "w"), ESFM_ERR_INVALID_ARG, "unknown metric 7");
    refused("width", check_metric_width(ctx, ESFM_HAMMING, 0, "descriptor width must be positive"), ESFM_ERR_INVALID_ARG, "descriptor width must be positive");
    accepted("metric and width", check_metric_width(ctx, ESFM_HAMMING, 32, "w"));
    for (int w : {16, 32, 64}) accepted("hamming width", check_hamming_width(ESFM_HAMMING, w));
    accepted("any L2 width", check_hamming_width(ESFM_L2_F32, 33));
    refused("hamming width 33", check_hamming_width(ESFM_HAMMING, 33), ESFM_ERR_UNSUPPORTED, "hamming descriptors must be 16, 32 or 64 bytes (got 33)");
    g_case = "row bytes";
    REQUIRE(match_row_bytes(ESFM_L2_F32, 64) == 256 && match_row_bytes(ESFM_HAMMING, 32) == 32, "row bytes");
}

}  // namespace

int main()
{
    // sizes one below, equal to and one above each query block (128, 256, 512), empty sets, and a set paired with itself
    const std::vector<int32_t> edge = {127, 128, 129, 0, 255, 256, 257, 511, 512, 513, 0, 1, 1025};
    std::vector<int32_t> all;
    for (int i = 0; i < (int)edge.size(); ++i)
        for (int j = 0; j <= i; ++j) { all.push_back(i); all.push_back(j); }      // j == i: the set with itself
    run("edge sizes, the pair loop", edge, all);
    run("no pairs", edge, {});
    run("only empty sets", {0, 0, 0}, {1, 0, 2, 1, 0, 0});
    run("one set", {300}, {0, 0});
    std::mt19937 rng(20240917u);
    for (int trial = 0; trial < 40; ++trial) {
        const int n_sets = 1 + (int)(rng() % 9u);
        std::vector<int32_t> sizes((size_t)n_sets);
        for (auto &s : sizes) {
            const unsigned k = rng() % 8u;
            s = k == 0 ? 0 : k == 1 ? (int32_t)(128 * (1 + rng() % 8u)) + (int32_t)(rng() % 3u) - 1 : (int32_t)(rng() % 3000u);
        }
        std::vector<int32_t> pairs(2 * (size_t)(rng() % 40u));
        for (auto &s : pairs) s = (int32_t)(rng() % (unsigned)n_sets);      // repeated pairs, repeated train sets (by_train's ties), self pairs
        run(("seeded " + std::to_string(trial)).c_str(), sizes, pairs);
    }
    limits();
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("match plan ok\n");
    return 0;
}
