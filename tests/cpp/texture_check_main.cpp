// The host-only half of the mesh texturing (easysfm_amd/csrc/texture_check.hpp) as a program of its own, built with g++ alone and
// run under AddressSanitizer + UBSan by tests/test_mesh_texture_cpu.py: every rejection path reads exactly the arrays it is given
// (they are heap blocks of exactly the stated size), the uv corners stay inside their squares, and the scratch layout keeps its
// arrays apart and inside the totals.  With a directory as its argument it also writes PNG files there with the host layer's writer
// (easysfm_amd/host/esfm_png.hpp, stored deflate blocks) and reads them back with its reader.  Needs -lz.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "../../easysfm_amd/host/esfm_png.hpp"
#include "texture_check.hpp"

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
    std::vector<float> score = std::vector<float>(3), uv = std::vector<float>(18);
    std::vector<uint8_t> atlas = std::vector<uint8_t>(10 * 10 * 3);
    esfm_mesh_texture_options opt{0.2f, 0.02f};
    int V = 4, T = 3, n = 2, rows = 12, cols = 16, channels = 3, S = 5, A = 2, cap = 10;
    int32_t atlas_rows = -7;
    bool with_opt = true, with_label = true, with_rows = true, with_images = true;
    int H = -7;
    int views()
    {
        return esfm::texture_check_views_args(V, T, vertices.empty() ? nullptr : vertices.data(), tri.empty() ? nullptr : tri.data(), n, rows, cols,
                                              K4.empty() ? nullptr : K4.data(), poses.data(), with_opt ? &opt : nullptr, with_label ? label.data() : nullptr,
                                              score.data());
    }
    int bake()
    {
        return esfm::texture_check_bake_args(V, T, vertices.empty() ? nullptr : vertices.data(), tri.empty() ? nullptr : tri.data(),
                                             with_label ? label.data() : nullptr, n, rows, cols, channels, with_images ? images.data() : nullptr, K4.data(),
                                             poses.data(), S, A, cap, atlas.data(), uv.data(), with_rows ? &atlas_rows : nullptr, &H);
    }
};

static void rejected(Case c, bool bake, const char *message)
{
    esfm::g_err[0] = 0;
    const int rc = bake ? c.bake() : c.views();
    if (rc != ESFM_ERR_INVALID_ARG || !std::strstr(esfm::g_err, message)) { ++failures; std::printf("expected \"%s\", got %d \"%s\"\n", message, rc, esfm::g_err); }
    if (c.H != -7 || c.atlas_rows != -7) { ++failures; std::printf("\"%s\": a rejection wrote the height\n", message); }
}

// rows x cols x 3 bytes through write_rgb and read_bgr: the same pixels, channels reversed
static void png_round_trip(const std::string &dir, int rows, int cols)
{
    std::vector<uint8_t> rgb(size_t(rows) * cols * 3), bgr;
    uint32_t x = 12345u + uint32_t(rows) * 7919u + uint32_t(cols);
    for (uint8_t &b : rgb) { x = x * 1664525u + 1013904223u; b = uint8_t(x >> 24); }
    const std::string path = dir + "/t_" + std::to_string(rows) + "x" + std::to_string(cols) + ".png";
    const std::string e = p3dv::png::write_rgb(path, rows, cols, rgb.data());
    if (!e.empty()) { ++failures; std::printf("write_rgb: %s\n", e.c_str()); return; }
    int r = 0, c = 0;
    const std::string e2 = p3dv::png::read_bgr(path, r, c, bgr);
    if (!e2.empty() || r != rows || c != cols || bgr.size() != rgb.size()) { ++failures; std::printf("read_bgr %dx%d: %s\n", rows, cols, e2.c_str()); return; }
    for (size_t k = 0; k < rgb.size(); k += 3)
        if (bgr[k] != rgb[k + 2] || bgr[k + 1] != rgb[k + 1] || bgr[k + 2] != rgb[k]) { ++failures; std::printf("pixel %zu of %dx%d differs\n", k / 3, rows, cols); return; }
}

int main(int argc, char **argv)
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    { Case c; EXPECT(c.views() == ESFM_OK); EXPECT(c.bake() == ESFM_OK && c.H == 5); }
    { Case c; c.V = 0; c.T = 0; EXPECT(c.views() == ESFM_OK); EXPECT(c.bake() == ESFM_OK && c.H == 0); }
    { Case c; c.cap = 3; EXPECT(c.bake() == ESFM_OK && c.H == 5); }          // (the capacity is the caller's to compare)
    for (int bake = 0; bake < 2; ++bake) {
        { Case c; c.vertices[7] = nan; rejected(c, bake, "a vertex is not finite"); }
        { Case c; c.vertices[11] = -inf; rejected(c, bake, "a vertex is not finite"); }
        { Case c; c.tri[4] = 4; rejected(c, bake, "triangle index"); }
        { Case c; c.tri[0] = -1; rejected(c, bake, "triangle index"); }
        { Case c; c.V = 3; rejected(c, bake, "triangle index"); }
        { Case c; c.V = -1; rejected(c, bake, "n_vertices"); }
        { Case c; c.T = -1; rejected(c, bake, "n_triangles"); }
        { Case c; c.T = (1 << 25) + 1; rejected(c, bake, "n_triangles"); }
        { Case c; c.vertices.clear(); rejected(c, bake, "NULL argument"); }
        { Case c; c.tri.clear(); rejected(c, bake, "NULL argument"); }
        { Case c; c.with_label = false; rejected(c, bake, "NULL argument"); }
        { Case c; c.n = 0; rejected(c, bake, "n_views"); }
        { Case c; c.n = 65; rejected(c, bake, "n_views"); }
        { Case c; c.rows = 1; rejected(c, bake, "rows and cols"); }
        { Case c; c.cols = 16385; rejected(c, bake, "rows and cols"); }
        { Case c; c.K4[5] = nan; rejected(c, bake, "K4 must be finite"); }
        { Case c; c.K4[6] = 0.f; rejected(c, bake, "focal length"); }
        { Case c; c.poses[23] = inf; rejected(c, bake, "poses must be finite"); }
    }
    { Case c; c.with_opt = false; rejected(c, false, "options are NULL"); }
    { Case c; c.opt.min_cos = 1.f; rejected(c, false, "min_cos"); }
    { Case c; c.opt.min_cos = -0.1f; rejected(c, false, "min_cos"); }
    { Case c; c.opt.min_cos = nan; rejected(c, false, "min_cos"); }
    { Case c; c.opt.min_cos = 0.f; c.opt.occlusion_tol = 0.f; EXPECT(c.views() == ESFM_OK); }
    { Case c; c.opt.occlusion_tol = 1.f; rejected(c, false, "occlusion_tol"); }
    { Case c; c.opt.occlusion_tol = nan; rejected(c, false, "occlusion_tol"); }
    { Case c; c.S = 3; rejected(c, true, "texels"); }
    { Case c; c.S = 65; rejected(c, true, "texels"); }
    { Case c; c.A = 0; rejected(c, true, "atlas_width"); }
    { Case c; c.A = 3277; rejected(c, true, "wider than 16384"); }
    { Case c; c.A = 3276; EXPECT(c.bake() == ESFM_OK && c.H == 5); }
    { Case c; c.label[1] = 2; rejected(c, true, "label"); }
    { Case c; c.label[2] = -2; rejected(c, true, "label"); }
    { Case c; c.channels = 2; rejected(c, true, "channels"); }
    { Case c; c.cap = -1; rejected(c, true, "max_atlas_rows"); }
    { Case c; c.with_rows = false; rejected(c, true, "NULL argument"); }
    { Case c; c.with_images = false; rejected(c, true, "NULL argument"); }
    // 513 triangles in one column of squares of 64 texels: 257 squares, 64 texels too high
    EXPECT(esfm::texture_atlas_rows(512, 64, 1) == 16384 && esfm::texture_atlas_rows(513, 64, 1) == -1 && std::strstr(esfm::g_err, "higher than 16384"));
    EXPECT(esfm::texture_atlas_rows(1 << 25, 4, 4096) == 16384 && esfm::texture_atlas_rows(0, 4, 1) == 0 && esfm::texture_atlas_rows(1, 4, 1) == 4);

    // uv: every corner strictly inside its square, at the stated offsets
    for (int S : {4, 5, 7, 64})
        for (int A : {1, 3})
            for (int T : {1, 2, 7, 12}) {
                const int H = esfm::texture_atlas_rows(T, S, A);
                std::vector<float> uv(6 * (size_t)T);
                esfm::texture_uv(T, S, A, H, uv.data());
                for (int t = 0; t < T; ++t)
                    for (int k = 0; k < 3; ++k) {
                        const double x = (double)uv[6 * t + 2 * k] * (A * S) - (t / 2 % A) * S, y = (double)uv[6 * t + 2 * k + 1] * H - (t / 2 / A) * S;
                        const double ex = t % 2 ? (k == 1 ? 2.5 : S - 0.5) : (k == 1 ? S - 1.5 : 0.5), ey = t % 2 ? (k == 2 ? 2.5 : S - 0.5) : (k == 2 ? S - 1.5 : 0.5);
                        EXPECT(x > 0 && x < S && y > 0 && y < S && std::fabs(x - ex) < 1e-3 && std::fabs(y - ey) < 1e-3);
                    }
            }

    // the layout: arrays in order, 256-byte aligned, apart, inside the totals; nothing for what a call does not use
    for (size_t V : {size_t(1), size_t(255), size_t(70001)})
        for (size_t T : {size_t(1), size_t(300), size_t(210000)})
            for (size_t n : {size_t(1), size_t(64)})
                for (int flags = 0; flags < 4; ++flags) {
                    const bool rgb = flags & 1, views = flags & 2;
                    const size_t pixels = views ? 180 * 240 : 0, image_bytes = views ? 0 : n * 180 * 240 * 3, atlas_bytes = views ? 0 : 12345;
                    const esfm::TextureLayout l = esfm::texture_layout(V, T, n, rgb, pixels, image_bytes, atlas_bytes);
                    const size_t a[] = {l.vertices, l.tri, l.rgb, l.cams, l.label, l.score, l.a_bytes};
                    const size_t need_a[] = {12 * V, 12 * T, rgb ? 3 * V : 0, 64 * n, 4 * T, 4 * T};
                    for (int k = 0; k < 6; ++k) EXPECT(a[k] % 256 == 0 && a[k] + need_a[k] <= a[k + 1]);
                    EXPECT(l.proj == 0 && l.proj + (views ? 16 * n * V : 0) <= l.buffers && l.buffers + 4 * n * pixels <= l.list &&
                           l.list + (views ? 4 * n * T : 0) <= l.count && l.count + (views ? 4 : 0) <= l.b_bytes && l.count % 256 == 0);
                    EXPECT(l.images == 0 && image_bytes <= l.c_bytes && l.atlas == 0 && atlas_bytes <= l.d_bytes);
                    EXPECT(views || l.b_bytes == 0);
                }
    EXPECT(sizeof(esfm::TextureCam) == 64);
    if (argc > 1) {
        // one pixel; a row of 65535 bytes with its filter byte (one stored block exactly); 65536 (two); many blocks; odd sizes
        for (const auto &rc : {std::pair<int, int>{1, 1}, {1, 21845}, {3, 21845}, {1, 21846}, {300, 251}, {7, 5}, {128, 128}}) png_round_trip(argv[1], rc.first, rc.second);
        EXPECT(!p3dv::png::write_rgb(std::string(argv[1]) + "/none.png", 0, 4, nullptr).empty());
        EXPECT(!p3dv::png::write_rgb(std::string(argv[1]) + "/no_such_dir/x.png", 1, 1, reinterpret_cast<const uint8_t *>("abc")).empty());
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("texture check ok\n");
    return 0;
}
