// The host-only half of the mesh rendering (easysfm_amd/csrc/render_check.hpp) as a program of its own, built with g++ alone and
// run under AddressSanitizer + UBSan by tests/test_mesh_render_cpu.py: every rejection path reads exactly the arrays it is given
// (they are heap blocks of exactly the stated size), and the scratch layout keeps its arrays apart and inside the totals.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "render_check.hpp"

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
    std::vector<float> uv = std::vector<float>(18, 0.5f);
    std::vector<uint8_t> atlas = std::vector<uint8_t>(2 * 3 * 3, 9);
    std::vector<float> K4{50.f, 7.5f, 50.f, 5.5f, 50.f, 7.5f, 50.f, 5.5f};
    std::vector<float> poses{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0.1f, 0, 1, 0, 0, 0, 0, 1, 0};
    std::vector<uint8_t> rgb = std::vector<uint8_t>(2 * 12 * 16 * 3, 7);
    std::vector<float> depth = std::vector<float>(2 * 12 * 16, 7.f);
    std::vector<int32_t> id = std::vector<int32_t>(2 * 12 * 16, 7);
    esfm_mesh_render_options opt{{1, 2, 3}, 0};
    int V = 4, T = 3, n = 2, rows = 12, cols = 16, H = 2, W = 3;
    bool with_opt = true, with_uv = true, with_atlas = true, with_rgb = true, with_depth = true, with_id = true;
    int check()
    {
        return esfm::render_check_args(V, T, vertices.empty() ? nullptr : vertices.data(), tri.empty() ? nullptr : tri.data(), with_uv ? uv.data() : nullptr, H, W,
                                       with_atlas ? atlas.data() : nullptr, n, rows, cols, K4.empty() ? nullptr : K4.data(), poses.data(),
                                       with_opt ? &opt : nullptr, with_rgb ? rgb.data() : nullptr, with_depth ? depth.data() : nullptr,
                                       with_id ? id.data() : nullptr);
    }
};

static void rejected(Case c, const char *message)
{
    esfm::g_err[0] = 0;
    const int rc = c.check();
    if (rc != ESFM_ERR_INVALID_ARG || !std::strstr(esfm::g_err, message)) { ++failures; std::printf("expected \"%s\", got %d \"%s\"\n", message, rc, esfm::g_err); }
    for (uint8_t b : c.rgb) if (b != 7) { ++failures; std::printf("\"%s\": a rejection wrote rgb\n", message); break; }
    for (float d : c.depth) if (d != 7.f) { ++failures; std::printf("\"%s\": a rejection wrote depth\n", message); break; }
    for (int32_t i : c.id) if (i != 7) { ++failures; std::printf("\"%s\": a rejection wrote triangle_id\n", message); break; }
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    { Case c; EXPECT(c.check() == ESFM_OK); }
    { Case c; c.with_uv = c.with_atlas = false; EXPECT(c.check() == ESFM_OK); }
    { Case c; c.V = 0; c.T = 0; EXPECT(c.check() == ESFM_OK); }
    { Case c; c.with_rgb = c.with_depth = false; EXPECT(c.check() == ESFM_OK); }
    { Case c; c.with_rgb = c.with_id = false; EXPECT(c.check() == ESFM_OK); }
    { Case c; c.with_depth = c.with_id = false; EXPECT(c.check() == ESFM_OK); }
    { Case c; c.with_rgb = c.with_depth = c.with_id = false; rejected(c, "all NULL"); }
    { Case c; c.with_opt = false; rejected(c, "options are NULL"); }
    { Case c; c.vertices[7] = nan; rejected(c, "a vertex is not finite"); }
    { Case c; c.vertices[11] = -inf; rejected(c, "a vertex is not finite"); }
    { Case c; c.tri[4] = 4; rejected(c, "triangle index"); }
    { Case c; c.tri[0] = -1; rejected(c, "triangle index"); }
    { Case c; c.V = 3; rejected(c, "triangle index"); }
    { Case c; c.V = -1; rejected(c, "n_vertices"); }
    { Case c; c.T = -1; rejected(c, "n_triangles"); }
    { Case c; c.T = (1 << 25) + 1; rejected(c, "n_triangles"); }
    { Case c; c.vertices.clear(); rejected(c, "NULL argument"); }
    { Case c; c.tri.clear(); rejected(c, "NULL argument"); }
    { Case c; c.n = 0; rejected(c, "n_views"); }
    { Case c; c.n = 65; rejected(c, "n_views"); }
    { Case c; c.rows = 1; rejected(c, "rows and cols"); }
    { Case c; c.cols = 16385; rejected(c, "rows and cols"); }
    { Case c; c.K4[5] = nan; rejected(c, "K4 must be finite"); }
    { Case c; c.K4[6] = 0.f; rejected(c, "focal length"); }
    { Case c; c.K4.clear(); rejected(c, "NULL argument"); }
    { Case c; c.poses[23] = inf; rejected(c, "poses must be finite"); }
    { Case c; c.with_uv = false; rejected(c, "both"); }
    { Case c; c.with_atlas = false; rejected(c, "both"); }
    { Case c; c.uv[17] = nan; rejected(c, "texture coordinate"); }
    { Case c; c.uv[0] = inf; rejected(c, "texture coordinate"); }
    { Case c; c.H = 1; rejected(c, "atlas"); }
    { Case c; c.W = 16385; rejected(c, "atlas"); }
    { Case c; c.with_uv = c.with_atlas = false; c.H = 0; c.W = 0; EXPECT(c.check() == ESFM_OK); }   // (the sizes are not looked at without an atlas)

    // the layout: arrays in order, 256-byte aligned, apart, inside the totals; nothing for what a call does not use
    for (size_t V : {size_t(1), size_t(255), size_t(70001)})
        for (size_t T : {size_t(1), size_t(300), size_t(210000)})
            for (size_t n : {size_t(1), size_t(64)})
                for (int flags = 0; flags < 32; ++flags) {
                    const bool rgb = flags & 1, tex = flags & 2, o_rgb = flags & 4, o_depth = flags & 8, o_id = flags & 16;
                    const size_t pixels = 180 * 240, atlas_bytes = tex ? 12345 : 0;
                    const esfm::RenderLayout l = esfm::render_layout(V, T, n, pixels, rgb, atlas_bytes, o_rgb, o_depth, o_id);
                    const size_t a[] = {l.vertices, l.tri, l.rgb, l.uv, l.cams, l.a_bytes};
                    const size_t need_a[] = {12 * V, 12 * T, rgb ? 3 * V : 0, tex ? 24 * T : 0, 64 * n};
                    for (int k = 0; k < 5; ++k) EXPECT(a[k] % 256 == 0 && a[k] + need_a[k] <= a[k + 1]);
                    EXPECT(l.proj == 0 && l.proj + 16 * n * V <= l.keys && l.keys % 256 == 0 && l.keys + 8 * n * pixels <= l.list && l.list + 4 * n * T <= l.count &&
                           l.count + 4 <= l.b_bytes && l.count % 256 == 0);
                    EXPECT(l.atlas == 0 && atlas_bytes <= l.c_bytes && (tex || l.c_bytes == 0));
                    EXPECT(l.out_rgb == 0 && l.out_rgb + (o_rgb ? 3 * n * pixels : 0) <= l.out_depth && l.out_depth % 256 == 0 &&
                           l.out_depth + (o_depth ? 4 * n * pixels : 0) <= l.out_id && l.out_id % 256 == 0 && l.out_id + (o_id ? 4 * n * pixels : 0) <= l.d_bytes);
                    EXPECT((o_rgb || o_depth || o_id) || l.d_bytes == 0);
                }
    EXPECT(sizeof(esfm_mesh_render_options) == 4);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("render check ok\n");
    return 0;
}
