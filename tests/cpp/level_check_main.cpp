// The host-only half of the seam levelling (easysfm_amd/csrc/level_check.hpp) as a program of its own, built with g++ alone and run
// under AddressSanitizer + UBSan by tests/test_mesh_texture_level_cpu.py: every rejection path reads exactly the arrays it is given
// (they are heap blocks of exactly the stated size), the host's tree_sum is the written loop and close to a long double sum, the
// stopping rule is the header's, and the scratch layout keeps its arrays apart and inside the totals.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "level_check.hpp"

namespace esfm {
static char g_err[1024];
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char *get_error() { return g_err; }
}  // namespace esfm

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { ++failures; std::printf("line %d: %s\n", __LINE__, #cond); } \
    } while (0)

struct Case {
    std::vector<float> vertices{0.f, 0.f, 2.f, 1.f, 0.f, 2.f, 0.f, 1.f, 2.f, 1.f, 1.f, 2.f};
    std::vector<int32_t> tri{0, 2, 1, 1, 2, 3, 0, 3, 1};
    std::vector<int32_t> label{0, 1, -1};
    std::vector<float> K4{50.f, 7.5f, 50.f, 5.5f, 50.f, 7.5f, 50.f, 5.5f};
    std::vector<float> poses{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0.1f, 0, 1, 0, 0, 0, 0, 1, 0};
    std::vector<uint8_t> images = std::vector<uint8_t>(2 * 12 * 16 * 3, 9);
    std::vector<float> offsets = std::vector<float>(27, 0.f);
    esfm_mesh_texture_level_options opt{0.1, 0.001, 1e-4, 200};
    esfm_mesh_texture_level_stats stats{-7, -7, -7, -7};
    int V = 4, T = 3, n = 2, rows = 12, cols = 16, channels = 3;
    bool with_opt = true, with_label = true, with_images = true, with_offsets = true, with_stats = true;
    int level()
    {
        return esfm::level_check_args(V, T, vertices.empty() ? nullptr : vertices.data(), tri.empty() ? nullptr : tri.data(), with_label ? label.data() : nullptr, n,
                                      rows, cols, channels, with_images ? images.data() : nullptr, K4.data(), poses.data(), with_opt ? &opt : nullptr,
                                      with_offsets ? offsets.data() : nullptr, with_stats ? &stats : nullptr);
    }
};

static void rejected(Case c, const char *message)
{
    esfm::g_err[0] = 0;
    const int rc = c.level();
    if (rc != ESFM_ERR_INVALID_ARG || !std::strstr(esfm::g_err, message)) { ++failures; std::printf("expected \"%s\", got %d \"%s\"\n", message, rc, esfm::g_err); }
    if (c.stats.nodes != -7 || c.stats.converged != -7) { ++failures; std::printf("\"%s\": a rejection wrote the stats\n", message); }
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const float finf = std::numeric_limits<float>::infinity(), fnan = std::numeric_limits<float>::quiet_NaN();
    { Case c; EXPECT(c.level() == ESFM_OK); }
    { Case c; c.V = 0; c.T = 0; c.with_label = false; c.with_offsets = false; EXPECT(c.level() == ESFM_OK); }
    { Case c; c.opt.tolerance = 0.0; c.opt.max_iterations = 0; EXPECT(c.level() == ESFM_OK); }
    { Case c; c.opt.max_iterations = 10000; c.channels = 1; EXPECT(c.level() == ESFM_OK); }
    { Case c; c.with_opt = false; rejected(c, "options are NULL"); }
    { Case c; c.opt.lambda = 0.0; rejected(c, "lambda"); }
    { Case c; c.opt.lambda = -0.1; rejected(c, "lambda"); }
    { Case c; c.opt.lambda = inf; rejected(c, "lambda"); }
    { Case c; c.opt.lambda = nan; rejected(c, "lambda"); }
    { Case c; c.opt.mu = 0.0; rejected(c, "mu"); }
    { Case c; c.opt.mu = nan; rejected(c, "mu"); }
    { Case c; c.opt.mu = inf; rejected(c, "mu"); }
    { Case c; c.opt.tolerance = 1.0; rejected(c, "tolerance"); }
    { Case c; c.opt.tolerance = -1e-12; rejected(c, "tolerance"); }
    { Case c; c.opt.tolerance = nan; rejected(c, "tolerance"); }
    { Case c; c.opt.max_iterations = -1; rejected(c, "max_iterations"); }
    { Case c; c.opt.max_iterations = 10001; rejected(c, "max_iterations"); }
    { Case c; c.with_stats = false; rejected(c, "NULL argument"); }
    { Case c; c.with_label = false; rejected(c, "NULL argument"); }
    { Case c; c.with_offsets = false; rejected(c, "NULL argument"); }
    { Case c; c.with_images = false; rejected(c, "NULL argument"); }
    { Case c; c.vertices.clear(); rejected(c, "NULL argument"); }
    { Case c; c.channels = 2; rejected(c, "channels"); }
    { Case c; c.vertices[7] = fnan; rejected(c, "a vertex is not finite"); }
    { Case c; c.tri[4] = 4; rejected(c, "triangle index"); }
    { Case c; c.T = (1 << 25) + 1; rejected(c, "n_triangles"); }
    { Case c; c.n = 65; rejected(c, "n_views"); }
    { Case c; c.rows = 1; rejected(c, "rows and cols"); }
    { Case c; c.K4[6] = 0.f; rejected(c, "focal length"); }
    { Case c; c.poses[23] = finf; rejected(c, "poses must be finite"); }
    { Case c; c.label[1] = 2; rejected(c, "label"); }
    { Case c; c.label[2] = -2; rejected(c, "label"); }

    // the offsets of the bake: exactly 9 T values are read
    {
        std::vector<float> o(27, 1.5f);
        EXPECT(esfm::level_check_offsets(3, o.data()) == ESFM_OK && esfm::level_check_offsets(3, nullptr) == ESFM_OK && esfm::level_check_offsets(0, o.data()) == ESFM_OK);
        for (float bad : {finf, -finf, fnan}) {
            o[26] = bad;
            EXPECT(esfm::level_check_offsets(3, o.data()) == ESFM_ERR_INVALID_ARG && std::strstr(esfm::g_err, "offset is not finite"));
            EXPECT(esfm::level_check_offsets(2, o.data()) == ESFM_OK);
        }
    }

    // tree_sum: the written loop on 600 values, exact on integers, close to a long double sum over the lengths that change the number of levels
    {
        std::vector<double> x(600);
        uint32_t s = 12345u;
        for (double &v : x) { s = s * 1664525u + 1013904223u; v = ((double)(s >> 8) / 8388608.0 - 1.0) * 1e3; }
        double level1[3] = {0.0, 0.0, 0.0};
        for (int b = 0; b < 3; ++b) {
            double blk[256];
            for (int i = 0; i < 256; ++i) blk[i] = 256 * b + i < 600 ? x[256 * b + i] : 0.0;
            for (int h = 128; h >= 1; h /= 2)
                for (int i = 0; i < h; ++i) blk[i] += blk[i + h];
            level1[b] = blk[0];
        }
        // the second level: 3 values and 253 zeros; the halving leaves (l0 + l2) + l1
        EXPECT(esfm::level_tree_sum(x.data(), 600) == (level1[0] + level1[2]) + level1[1]);
        EXPECT(esfm::level_tree_sum(x.data(), 0) == 0.0 && esfm::level_tree_sum(x.data(), 1) == x[0]);
        for (size_t n : {size_t(255), size_t(256), size_t(257), size_t(65536), size_t(65537)}) {
            std::vector<double> y(n);
            long double exact = 0.0L;
            double count = 0.0;
            for (size_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; y[i] = (double)(s >> 8) / 8388608.0 + 0.25; exact += y[i]; count += 1.0; }
            const double got = esfm::level_tree_sum(y.data(), n);
            EXPECT(std::fabs((double)((long double)got - exact)) <= 1e-12 * (double)exact);
            std::vector<double> ones(n, 1.0);
            EXPECT(esfm::level_tree_sum(ones.data(), n) == count);
        }
    }

    // the stopping rule: every channel, <=, and a NaN never stops
    {
        const double bb[3] = {4.0, 0.0, 1.0};
        const double ok[3] = {4e-8, 0.0, 1e-8}, one[3] = {4e-8, 1e-300, 1e-8}, bad[3] = {nan, 0.0, 0.0};
        EXPECT(esfm::level_converged(ok, bb, 1e-4) && !esfm::level_converged(one, bb, 1e-4) && !esfm::level_converged(bad, bb, 1e-4));
        EXPECT(!esfm::level_converged(ok, bb, 0.0));
    }
    EXPECT(esfm::bit_width(0) == 0 && esfm::bit_width(1) == 1 && esfm::bit_width(255) == 8 && esfm::bit_width(256) == 9);

    // the layout: arrays in order, 256-byte aligned, apart, inside the totals
    for (size_t V : {size_t(1), size_t(255), size_t(70001)})
        for (size_t T : {size_t(1), size_t(86), size_t(300), size_t(210000)})
            for (size_t n : {size_t(1), size_t(64)}) {
                const size_t image_bytes = n * 180 * 240 * 3, sort_bytes = 12345;
                const esfm::LevelLayout l = esfm::level_layout(V, T, n, image_bytes, sort_bytes);
                const size_t C3 = 3 * T;
                EXPECT(l.corners == C3 && l.stride >= C3 && l.stride % 256 == 0 && l.stride < C3 + 256 && l.partials * 256 >= l.stride && l.partials % 256 == 0);
                const size_t a[] = {l.vertices, l.tri, l.label, l.cams, l.a_bytes};
                const size_t need_a[] = {12 * V, 12 * T, 4 * T, 64 * n};
                for (int k = 0; k < 4; ++k) EXPECT(a[k] % 256 == 0 && a[k] + need_a[k] <= a[k + 1]);
                const size_t b[] = {l.keys, l.sorted, l.head_rank, l.head_blocks, l.sort, l.b_bytes};
                const size_t need_b[] = {48 * T, 48 * T, 4 * (6 * T + 1), 4 * ((6 * T + 255) / 256 + 1), sort_bytes};
                for (int k = 0; k < 5; ++k) EXPECT(b[k] % 256 == 0 && b[k] + need_b[k] <= b[k + 1]);
                EXPECT(l.images == 0 && image_bytes <= l.c_bytes);
                const size_t d[] = {l.corner_keys, l.node_keys, l.corner_node, l.seam_first, l.seam_last, l.col, l.row_start, l.pinned, l.f, l.d, l.g, l.r, l.p, l.q,
                                    l.part_a, l.part_b, l.scalars, l.counters, l.offsets, l.samples, l.d_bytes};
                const size_t need_d[] = {8 * C3, 8 * C3, 4 * C3, 4 * C3, 4 * C3, 24 * T, 4 * (C3 + 1), C3, 12 * l.stride, 8 * l.stride, 24 * l.stride, 24 * l.stride,
                                         24 * l.stride, 24 * l.stride, 24 * l.partials, 24 * l.partials, 8 * esfm::kLevelScalars, 16, 36 * T, 36 * T};
                for (int k = 0; k < 20; ++k) EXPECT(d[k] % 256 == 0 && d[k] + need_d[k] <= d[k + 1]);
            }
    EXPECT(sizeof(esfm_mesh_texture_level_options) == 32 && sizeof(esfm_mesh_texture_level_stats) == 16);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("level check ok\n");
    return 0;
}
