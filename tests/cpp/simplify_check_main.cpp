// The host-only half of esfm_mesh_simplify (easysfm_amd/csrc/simplify_check.hpp) as a program of its own, built with g++ alone and
// run under AddressSanitizer + UBSan by tests/test_mesh_simplify_cpu.py: every rejection path reads exactly the arrays it is given
// (they are heap blocks of exactly the stated size) and the scratch layout keeps its arrays apart and inside the totals.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "simplify_check.hpp"

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
    std::vector<float> vertices{0.1f, 0.1f, 0.1f, 1.2f, 0.1f, 0.2f, 0.2f, 1.3f, 0.1f, 1.1f, 1.2f, 1.3f};
    std::vector<uint8_t> rgb = std::vector<uint8_t>(12, 9);
    std::vector<int32_t> tri{0, 1, 2, 2, 1, 3};
    std::vector<float> out_v = std::vector<float>(12), origin{0.f, 0.f, 0.f};
    std::vector<uint8_t> out_c = std::vector<uint8_t>(12);
    std::vector<int32_t> out_t = std::vector<int32_t>(6);
    esfm_mesh_simplify_options opt{1e-3f, 1};
    float cell = 1.f;
    int V = 4, T = 2;
    int32_t nv = 5, nt = 5;
    bool with_rgb = true, with_out_rgb = true, with_opt = true, with_counts = true;
    int run() const
    {
        return esfm::simplify_check_args(V, T, vertices.empty() ? nullptr : vertices.data(), with_rgb ? rgb.data() : nullptr, tri.empty() ? nullptr : tri.data(),
                                         origin.empty() ? nullptr : origin.data(), cell, with_opt ? &opt : nullptr, out_v.data(),
                                         with_out_rgb ? out_c.data() : nullptr, out_t.data(), with_counts ? &nv : nullptr, &nt);
    }
};

static void rejected(const Case &c, const char *message)
{
    esfm::g_err[0] = 0;
    const int rc = c.run();
    if (rc != ESFM_ERR_INVALID_ARG || !std::strstr(esfm::g_err, message)) { ++failures; std::printf("expected \"%s\", got %d \"%s\"\n", message, rc, esfm::g_err); }
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    { Case c; EXPECT(c.run() == ESFM_OK); }
    { Case c; c.with_rgb = false; c.with_out_rgb = false; EXPECT(c.run() == ESFM_OK); }
    { Case c; c.V = 0; c.T = 0; EXPECT(c.run() == ESFM_OK); }
    { Case c; c.cell = 0.f; rejected(c, "cell"); }
    { Case c; c.cell = -1.f; rejected(c, "cell"); }
    { Case c; c.cell = nan; rejected(c, "cell"); }
    { Case c; c.cell = inf; rejected(c, "cell"); }
    { Case c; c.origin[1] = nan; rejected(c, "origin"); }
    { Case c; c.origin[2] = -inf; rejected(c, "origin"); }
    { Case c; c.origin.clear(); rejected(c, "NULL argument"); }
    { Case c; c.origin[0] = 0.5f; rejected(c, "outside the grid"); }                    // a vertex left of the origin
    { Case c; c.cell = 1e-7f; rejected(c, "outside the grid"); }                        // index 2^21 and beyond
    { Case c; c.vertices[7] = nan; rejected(c, "outside the grid"); }
    { Case c; c.vertices[11] = inf; rejected(c, "outside the grid"); }
    { Case c; c.cell = 1.3f / 2097151.f; c.vertices = {0.f, 0.f, 0.f, 1.2f, 0.1f, 0.2f, 0.2f, 1.29f, 0.1f, 1.1f, 1.2f, 1.29f}; EXPECT(c.run() == ESFM_OK); }
    { Case c; c.with_rgb = false; rejected(c, "output array is requested without its input"); }
    { Case c; c.with_opt = false; rejected(c, "options are NULL"); }
    { Case c; c.opt.regularisation = 0.f; rejected(c, "regularisation"); }
    { Case c; c.opt.regularisation = 1.5f; rejected(c, "regularisation"); }
    { Case c; c.opt.regularisation = nan; rejected(c, "regularisation"); }
    { Case c; c.opt.regularisation = 1.f; EXPECT(c.run() == ESFM_OK); }
    { Case c; c.opt.use_quadric = 2; rejected(c, "use_quadric"); }
    { Case c; c.opt.use_quadric = -1; rejected(c, "use_quadric"); }
    { Case c; c.tri[4] = 4; rejected(c, "triangle index"); }
    { Case c; c.tri[0] = -1; rejected(c, "triangle index"); }
    { Case c; c.V = 3; rejected(c, "triangle index"); }
    { Case c; c.V = -1; rejected(c, "n_vertices"); }
    { Case c; c.V = (1 << 30) + 1; c.T = 0; rejected(c, "n_vertices"); }
    { Case c; c.T = -1; rejected(c, "n_triangles"); }
    { Case c; c.T = (1 << 28) + 1; c.tri.clear(); rejected(c, "n_triangles"); }
    { Case c; c.vertices.clear(); rejected(c, "NULL argument"); }
    { Case c; c.tri.clear(); rejected(c, "NULL argument"); }
    { Case c; c.with_counts = false; rejected(c, "NULL argument"); }

    // the layout: arrays in order, 256-byte aligned, apart, inside the totals; nothing for what is not asked for
    for (size_t V : {size_t(1), size_t(255), size_t(256), size_t(70001)})
        for (size_t T : {size_t(1), size_t(300), size_t(210000)})
            for (int flags = 0; flags < 16; ++flags) {
                const bool rgb = flags & 1, normals = flags & 2, vmap = flags & 4, tmap = flags & 8;
                const esfm::SimplifyLayout l = esfm::simplify_layout(V, T, rgb, normals, vmap, tmap, 12345);
                const size_t a[] = {l.vertices, l.rgb, l.tri, l.cell_of, l.cell_start, l.cell_key, l.new_of_cell, l.used, l.keep, l.cell_blocks, l.used_blocks,
                                    l.tri_blocks, l.rep, l.rep_rgb, l.a_bytes};
                const size_t need_a[] = {12 * V, rgb ? 3 * V : 0, 12 * T, 4 * V, 4 * (V + 1), 8 * V, 4 * V, V, T, 4 * ((V + 255) / 256 + 1),
                                         4 * ((V + 255) / 256 + 1), 4 * ((T + 255) / 256 + 1), 12 * V, rgb ? 3 * V : 0};
                for (int k = 0; k < 14; ++k) EXPECT(a[k] % 256 == 0 && a[k] + need_a[k] <= a[k + 1]);
                const size_t keys = 3 * T > V ? 3 * T : V, vals = T > V ? T : V;
                EXPECT(l.key_in == 0 && l.key_in + 8 * keys <= l.key_out && l.key_out + 8 * keys <= l.val_in && l.val_in + 4 * vals <= l.val_out &&
                       l.val_out + 4 * vals <= l.sort && l.sort + 12345 <= l.b_bytes && l.sort % 256 == 0);
                EXPECT(l.inc_start + (normals ? 4 * (V + 1) : 0) <= l.face && l.face + (normals ? 12 * T : 0) <= l.c_bytes);
                EXPECT(l.out_vertices + 12 * V <= l.out_normals && l.out_normals + (normals ? 12 * V : 0) <= l.out_rgb && l.out_rgb + (rgb ? 3 * V : 0) <= l.out_tri &&
                       l.out_tri + 12 * T <= l.vertex_map && l.vertex_map + (vmap ? 4 * V : 0) <= l.triangle_map && l.triangle_map + (tmap ? 4 * T : 0) <= l.d_bytes);
            }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("simplify check ok\n");
    return 0;
}
