// Stand-alone host check of image retrieval's host code (no GPU call is made): easysfm_amd/csrc/retrieval_host.hpp -- the option
// rules, the training sample's arithmetic and the pair list -- compiled into this program so that -fsanitize=address,undefined sees
// every index it forms.  The pair-list cases are those of tests/test_retrieval_cpu.py: the window alone, a table with -1 padding,
// duplicates in both directions, a window beyond the number of sets, a single set, and a list that fills its capacity exactly
// (the output buffers here have exactly the documented capacity, so one entry too many is a heap overflow the sanitizer reports).
// Built by tests/test_retrieval_cpu.py, once plainly and once with the sanitizers.
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "../../easysfm_amd/csrc/retrieval_host.hpp"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

namespace {

namespace R = esfm::retrieval;

// the rule, restated with a std::set
std::vector<int32_t> expected(int n, int top_k, const std::vector<int32_t> &nearest, int window)
{
    std::set<std::pair<int, int>> chosen;
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < top_k; ++k) {
            const int j = nearest[size_t(i) * size_t(top_k) + size_t(k)];
            if (j >= 0) chosen.insert({i > j ? i : j, i > j ? j : i});
        }
        for (int w = 1; w <= window && i - w >= 0; ++w) chosen.insert({i, i - w});
    }
    std::vector<int32_t> out;
    for (const auto &p : chosen) { out.push_back(p.first); out.push_back(p.second); }
    return out;
}

int run_case(int n, int top_k, const std::vector<int32_t> &nearest, int window, size_t want_pairs)
{
    const int reach = window < n ? window : n;             // the documented capacity, with the window clipped to what can occur
    std::vector<int32_t> pairs(2 * size_t(n) * size_t(top_k + reach));
    int32_t count = -1;
    const char *why = nullptr;
    CHECK(R::pair_list(n, top_k, top_k ? nearest.data() : nullptr, window, pairs.data(), &count, &why) == ESFM_OK);
    const std::vector<int32_t> want = expected(n, top_k, nearest, window);
    CHECK(size_t(count) * 2 == want.size() && size_t(count) == want_pairs);
    for (size_t e = 0; e < want.size(); ++e) CHECK(pairs[e] == want[e]);
    for (int p = 0; p + 1 < count; ++p)
        CHECK(pairs[2 * p] < pairs[2 * p + 2] || (pairs[2 * p] == pairs[2 * p + 2] && pairs[2 * p + 1] < pairs[2 * p + 3]));
    return 0;
}

}  // namespace

int main()
{
    if (run_case(5, 0, {}, 2, 7)) return 1;                                              // the window alone
    if (run_case(4, 2, {1, -1, -1, -1, 0, 1, 2, -1}, 0, 4)) return 1;                     // -1 padding
    if (run_case(4, 2, {1, 2, 0, 3, 0, 1, 1, 0}, 1, 6)) return 1;                         // (i -> j) and (j -> i), and the window's pairs again
    if (run_case(4, 1, {3, -1, -1, -1}, 9, 6)) return 1;                                  // window >= n_sets: every pair
    if (run_case(1, 3, {-1, -1, -1}, 2, 0)) return 1;                                     // one set: the empty list
    if (run_case(3, 1, {1, 2, 0}, 0, 3)) return 1;                                        // capacity exactly reached
    if (run_case(0, 4, {}, 3, 0)) return 1;

    // rejected, nothing written
    int32_t guard[4] = {-7, -7, -7, -7}, count = -7;
    const char *why = nullptr;
    const int32_t own_row[2] = {0, 0}, beyond[2] = {1, 2}, below[2] = {-2, 0};
    for (const int32_t *bad : {own_row, beyond, below}) {
        CHECK(R::pair_list(2, 1, bad, 0, guard, &count, &why) == ESFM_ERR_INVALID_ARG && why);
        CHECK(count == -7 && guard[0] == -7 && guard[1] == -7);
    }
    CHECK(R::pair_list(2, 1, nullptr, 0, guard, &count, &why) == ESFM_ERR_INVALID_ARG);
    CHECK(R::pair_list(2, -1, own_row, 0, guard, &count, &why) == ESFM_ERR_INVALID_ARG);
    CHECK(R::pair_list(2, 0, nullptr, -1, guard, &count, &why) == ESFM_ERR_INVALID_ARG);
    CHECK(R::pair_list(-1, 0, nullptr, 0, guard, &count, &why) == ESFM_ERR_INVALID_ARG);
    CHECK(R::pair_list(2, 0, nullptr, 1, guard, nullptr, &why) == ESFM_ERR_INVALID_ARG);

    // the option rules and the sample
    esfm_retrieval_options o = {64, 10, 65536, 10, 0, 0};
    CHECK(!R::options_error(&o) && R::options_error(nullptr));
    for (int v : {0, 257}) { esfm_retrieval_options b = o; b.n_centres = v; CHECK(R::options_error(&b)); }
    { esfm_retrieval_options b = o; b.top_k = -1; CHECK(R::options_error(&b)); b.top_k = 1025; CHECK(R::options_error(&b)); }
    { esfm_retrieval_options b = o; b.kmeans_iterations = 101; CHECK(R::options_error(&b)); b.kmeans_iterations = 0; CHECK(!R::options_error(&b)); }
    { esfm_retrieval_options b = o; b.max_train = 0; CHECK(R::options_error(&b)); b.max_train = (1 << 24) + 1; CHECK(R::options_error(&b)); }
    { esfm_retrieval_options b = o; b.window = -1; CHECK(R::options_error(&b)); }
    int64_t stride = 0, nt = 0;
    R::train_sample(10, 4, &stride, &nt); CHECK(stride == 3 && nt == 4);
    R::train_sample(10, 10, &stride, &nt); CHECK(stride == 1 && nt == 10);
    R::train_sample(7, 100, &stride, &nt); CHECK(stride == 1 && nt == 7);
    R::train_sample(2147483647, 1 << 24, &stride, &nt); CHECK(stride == 128 && nt == 16777216);
    CHECK(R::working_dim(ESFM_L2_F32, 256) == 256 && R::working_dim(ESFM_L2_F32, 257) == 0 && R::working_dim(ESFM_HAMMING, 64) == 512
          && R::working_dim(ESFM_HAMMING, 65) == 0 && R::working_dim(ESFM_HAMMING, 0) == 0);
    const int32_t up[3] = {0, 4, 4}, down[3] = {0, 4, 2};
    CHECK(!R::offsets_error(up, 2) && R::offsets_error(down, 2) && R::offsets_error(nullptr, 2));
    std::printf("retrieval check ok\n");
    return 0;
}
