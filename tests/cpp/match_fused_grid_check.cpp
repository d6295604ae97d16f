// What l2_fused_kernel (easysfm_amd/csrc/match_kernels.hip) relies on in the pair plan and in the fused launch's grid arithmetic
// (match_plan.hpp: fused_grid_of, pair_blocks2), checked on the CPU (tests/test_match_fused_plan.py builds this against match_plan.cpp
// alone).  The kernel derives every role from its workgroup index with the same three comparisons this program walks through.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "match_plan.hpp"

using namespace esfm;

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

constexpr int kQueryBlock2 = 512;      // l2_x1_query_block(): queries per pass block

// xcd_remap of match_device.hpp: XCD x = bid % 8 owns a contiguous range of the logical numbering
int xcd_remap(int bid, int nb)
{
    const int q = nb >> 3, r = nb & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

void check(const char *name, const std::vector<int32_t> &sizes, const std::vector<int32_t> &pairs, bool walk)
{
    g_case = name;
    std::vector<int32_t> off(sizes.size() + 1, 0);
    for (size_t s = 0; s < sizes.size(); ++s) off[s + 1] = off[s] + sizes[s];
    const int P = (int)(pairs.size() / 2);
    std::vector<int64_t> out_offset((size_t)P + 1);
    PairPlan plan;
    const int rc = make_plan(off.data(), (int)sizes.size(), pairs.data(), P, 256, kQueryBlock2, false, kPlainPlanRules, out_offset.data(), &plan);
    REQUIRE(rc == ESFM_OK, "rc %d: %s", rc, g_error.c_str());

    // ---- the hand-over's target: a pair's finish workgroups wait for pair_blocks2() counts, and exactly that many pass blocks name
    // the pair in blk_pair (each of them adds 1 to pass_done[pair], nobody else does)
    std::vector<int> named((size_t)P, 0);
    for (int32_t g : plan.blk_pair) { REQUIRE(g >= 0 && g < P, "blk_pair entry %d", g); ++named[(size_t)g]; }
    int64_t sum = 0;
    for (int p = 0; p < P; ++p) {
        const PairDesc &d = plan.tab[(size_t)p];
        const int need = pair_blocks2(d, kQueryBlock2);
        REQUIRE(need == named[(size_t)p], "pair %d: waits for %d blocks, %d name it", p, need, named[(size_t)p]);
        REQUIRE(need == (p + 1 < P ? plan.tab[(size_t)p + 1].blk_off2 : plan.n_blocks2) - d.blk_off2, "pair %d: blk_off2 difference", p);
        REQUIRE((need == 0) == (d.nq == 0), "pair %d: a pair waits for nothing exactly when it has no query", p);
        REQUIRE(need == (d.nq + kQueryBlock2 - 1) / kQueryBlock2, "pair %d: %d blocks for %d queries and %d train rows", p, need, d.nq, d.nt);   // (whatever nt is: an empty train set's blocks exist and count)
        sum += need;
    }
    REQUIRE(sum == plan.n_blocks2, "block total");

    // ---- the grid
    const int S = fused_slices_default(P);
    REQUIRE(S >= 1 && S <= 8, "slices %d", S);
    const FusedGrid g = fused_grid_of(plan.n_blocks2, P, S);
    REQUIRE(g.n_pass == plan.n_blocks2 && g.slices == S, "echo");
    REQUIRE(g.n_pad % 8 == 0 && g.n_pad >= g.n_pass && g.n_pad - g.n_pass < 8, "padding: %lld behind %d", (long long)g.n_pad, g.n_pass);
    REQUIRE(g.total == g.n_pad + (int64_t)P * S, "total");
    if (!walk) return;
    // every workgroup of the grid has one role; the pass role covers every logical block once; the finish role covers every
    // (pair in by_train order, slice) once, and its workgroup k sits on the XCD a launch of its own would give it
    std::vector<char> blk_seen((size_t)g.n_pass, 0), fin_seen((size_t)P * (size_t)S, 0);
    int64_t padding = 0, last_pass = -1, first_fin = g.total;
    for (int64_t w = 0; w < g.total; ++w) {
        if (w < g.n_pad) {
            if (w >= g.n_pass) { ++padding; continue; }
            const int lb = xcd_remap((int)w, g.n_pass);
            REQUIRE(lb >= 0 && lb < g.n_pass && !blk_seen[(size_t)lb], "pass block %d of workgroup %lld", lb, (long long)w);
            blk_seen[(size_t)lb] = 1;
            last_pass = std::max(last_pass, w);
        } else {
            first_fin = std::min(first_fin, w);
            const int fb = (int)(w - g.n_pad), nfb = P * S;
            REQUIRE(fb % 8 == (int)(w % 8), "finish workgroup %d is on XCD %d of the launch", fb, (int)(w % 8));
            const int lb = xcd_remap(fb, nfb);
            REQUIRE(lb >= 0 && lb < nfb && !fin_seen[(size_t)lb], "finish workgroup %d", fb);
            fin_seen[(size_t)lb] = 1;
            const int p = plan.by_train[(size_t)(lb / S)];
            REQUIRE(p >= 0 && p < P, "pair of finish workgroup %d", fb);
        }
    }
    REQUIRE(padding == g.n_pad - g.n_pass, "padding workgroups");
    // the progress argument's first line: every pass block has a lower workgroup index than every finish workgroup, and the finish
    // role starts on a multiple of 8
    REQUIRE(last_pass < first_fin && (first_fin == g.total || first_fin % 8 == 0), "role boundary: pass up to %lld, finish from %lld", (long long)last_pass, (long long)first_fin);
    for (char c : blk_seen) REQUIRE(c, "a pass block without a workgroup");
    for (char c : fin_seen) REQUIRE(c, "a finish slice without a workgroup");
}

}  // namespace

int main()
{
    // the degenerate lists of tests/test_match_fused_gpu.py
    check("one query", {2, 1}, {1, 0}, true);
    check("ragged: 513 x 300 / 200", {513, 300, 200}, {0, 1, 0, 2}, true);
    check("no queries / no train rows", {0, 100, 70}, {0, 1, 1, 0, 1, 2, 0, 0, 2, 1}, true);
    check("only pairs without queries", {0, 9}, {0, 1, 0, 0}, true);
    check("no pairs", {5, 5}, {}, true);
    for (size_t n_small : {(size_t)600, (size_t)2400}) {
        std::vector<int32_t> sizes = {2048, 2048}, pairs;
        for (int i = 0; i < 70; ++i) sizes.push_back(64);
        for (int i = 0; i < 70 && pairs.size() < 2 * n_small; ++i)
            for (int j = 0; j < i && pairs.size() < 2 * n_small; ++j) { pairs.push_back(2 + i); pairs.push_back(2 + j); }
        pairs.push_back(1); pairs.push_back(0);
        check("small pairs and a large one", sizes, pairs, true);
    }
    {   // block counts 0 .. 8 around the padding's period, every list length 1 .. 20
        std::vector<int32_t> sizes;
        for (int b = 0; b <= 8; ++b) { sizes.push_back(512 * b); sizes.push_back(512 * b + 1); }
        for (int n = 1; n <= 20; ++n) {
            std::vector<int32_t> pairs;
            for (int k = 0; k < n; ++k) { pairs.push_back((7 * k + n) % (int)sizes.size()); pairs.push_back((3 * k) % (int)sizes.size()); }
            check(("period " + std::to_string(n)).c_str(), sizes, pairs, true);
        }
    }
    {   // train sets of 65 535 rows (the largest a 16-bit count would hold; the pass numbers up to 65 536), all pairs of 40 sets
        std::vector<int32_t> sizes(40, 65535), pairs;
        for (int i = 0; i < 40; ++i)
            for (int j = 0; j < i; ++j) { pairs.push_back(i); pairs.push_back(j); }
        check("65 535-row sets", sizes, pairs, true);
    }
    {   // a list long enough for one finish workgroup per pair, and a grid near the launcher's limit (arithmetic only)
        std::vector<int32_t> sizes = {300, 700}, pairs;
        for (int k = 0; k < 3000; ++k) { pairs.push_back(k & 1); pairs.push_back(1 - (k & 1)); }
        check("3000 pairs", sizes, pairs, true);
        const FusedGrid g = fused_grid_of(2147483647, 1 << 20, 8);
        g_case = "large";
        if (!(g.n_pad == 2147483648LL && g.total == 2147483648LL + (8LL << 20))) { printf("FAIL [large] 64-bit arithmetic\n"); ++g_failed; }
    }
    std::mt19937 rng(20250211u);
    for (int trial = 0; trial < 40; ++trial) {
        const int n_sets = 1 + (int)(rng() % 9u);
        std::vector<int32_t> sizes((size_t)n_sets);
        for (auto &s : sizes) {
            const unsigned k = rng() % 6u;
            s = k == 0 ? 0 : k == 1 ? (int32_t)(512 * (1 + rng() % 4u)) + (int32_t)(rng() % 3u) - 1 : (int32_t)(rng() % 3000u);
        }
        std::vector<int32_t> pairs(2 * (size_t)(rng() % 60u));
        for (auto &s : pairs) s = (int32_t)(rng() % (unsigned)n_sets);
        check(("seeded " + std::to_string(trial)).c_str(), sizes, pairs, true);
    }
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("fused grid ok\n");
    return 0;
}
