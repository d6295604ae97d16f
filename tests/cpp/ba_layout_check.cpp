// What the bundle-adjustment kernels rely on in the index tables of easysfm_amd/csrc/ba_layout.cpp, checked on the CPU over seeded
// observation lists (tests/test_ba_layout.py builds this against ba_layout.cpp alone).  Each block names the kernel that reads
// the table and states what that kernel assumes without checking.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "ba_layout.hpp"

using namespace esfm;

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

struct Scene { int n_real = 0, n_pt = 0; std::vector<int32_t> cam, pt; };

// ring of cameras, every point seen by `len(p)` consecutive ring cameras from a random start (synth.ba_scene); camera-major order
template <class Len> Scene ring(int n_real, int n_pt, unsigned seed, Len len, bool camera_major = true)
{
    Scene s; s.n_real = n_real; s.n_pt = n_pt;
    std::mt19937 rng(seed);
    std::vector<std::pair<int32_t, int32_t>> obs;
    for (int p = 0; p < n_pt; ++p) {
        const int c0 = (int)(rng() % (unsigned)n_real), n = std::min(len(p, rng), n_real);
        for (int j = 0; j < n; ++j) obs.push_back({(c0 + j) % n_real, p});
    }
    if (camera_major) std::stable_sort(obs.begin(), obs.end());
    else std::shuffle(obs.begin(), obs.end(), rng);
    for (auto &o : obs) { s.cam.push_back(o.first); s.pt.push_back(o.second); }
    return s;
}

struct Span { int lo = INT32_MAX, hi = -1; int width() const { return hi - lo; } };

void check(const Scene &s, int num_cu, bool schur_tables)
{
    const int n_real = s.n_real, n_pt = s.n_pt, n_obs = (int)s.cam.size();
    const BaLayout L = make_ba_layout(n_real, n_pt, n_obs, s.cam.data(), s.pt.data(), num_cu, schur_tables);
    const size_t no = (size_t)n_obs;

    // ---- sort (every kernel: "obs k in [pt_start[p], pt_start[p+1]) belongs to point p"; the caller's order inside a point is what
    // makes a point's sums bit-reproducible against the CPU oracle) ----
    REQUIRE(L.order.size() == no && L.cam.size() == no && L.pt.size() == no && L.pt_start.size() == (size_t)n_pt + 1, "sizes");
    {
        std::vector<char> seen(no, 0);
        for (size_t t = 0; t < no; ++t) {
            const int k = L.order[t];
            REQUIRE(k >= 0 && k < n_obs && !seen[(size_t)k], "order is not a permutation at %zu", t);
            seen[(size_t)k] = 1;
            REQUIRE(L.cam[t] == s.cam[(size_t)k] && L.pt[t] == s.pt[(size_t)k], "sorted cam/pt at %zu", t);
            if (t) REQUIRE(L.pt[t - 1] < L.pt[t] || (L.pt[t - 1] == L.pt[t] && L.order[t - 1] < k), "not stable by point at %zu", t);
        }
        REQUIRE(L.pt_start[0] == 0 && L.pt_start[(size_t)n_pt] == n_obs, "pt_start ends");
        for (int p = 0; p < n_pt; ++p) {
            REQUIRE(L.pt_start[(size_t)p] <= L.pt_start[(size_t)p + 1], "pt_start decreases at %d", p);
            for (int t = L.pt_start[(size_t)p]; t < L.pt_start[(size_t)p + 1]; ++t) REQUIRE(L.pt[(size_t)t] == p, "pt_start is not the CSR at %d", t);
        }
        REQUIRE(L.cam_nobs.size() == (size_t)n_real, "cam_nobs size");
        std::vector<int32_t> cnt((size_t)n_real, 0);
        for (size_t t = 0; t < no; ++t) cnt[(size_t)L.cam[t]]++;
        long long total = 0;
        for (int c = 0; c < n_real; ++c) { REQUIRE(cnt[(size_t)c] == L.cam_nobs[(size_t)c], "cam_nobs[%d]", c); total += L.cam_nobs[(size_t)c]; }
        REQUIRE(total == n_obs, "cam_nobs sum");
    }
    auto pt_len = [&](int p) { return L.pt_start[(size_t)p + 1] - L.pt_start[(size_t)p]; };

    // ---- camera chunks (ba_camacc_chunk_kernel: one wave sums observations cam_obs[beg .. end) of ONE camera in index order;
    // ba_camacc_final_kernel adds chunks cam_chunk0[c] .. cam_chunk0[c + 1] in order) ----
    {
        const size_t nch = L.cchunk_cam.size();
        REQUIRE(L.cam_obs.size() == no && L.cchunk_beg.size() == nch && L.cchunk_end.size() == nch && L.cam_chunk0.size() == (size_t)n_real + 1, "sizes");
        std::vector<char> seen(no, 0);
        int next = 0;
        for (size_t b = 0; b < nch; ++b) {
            const int c = L.cchunk_cam[b], beg = L.cchunk_beg[b], end = L.cchunk_end[b];
            REQUIRE(c >= 0 && c < n_real && beg == next && beg < end && end <= n_obs && end - beg <= kCamChunk, "chunk %zu bounds", b);
            REQUIRE(b == 0 || L.cchunk_cam[b - 1] <= c, "chunk cameras descend at %zu", b);
            REQUIRE((int)b >= L.cam_chunk0[(size_t)c] && (int)b < L.cam_chunk0[(size_t)c + 1], "cam_chunk0 does not cover chunk %zu", b);
            for (int i = beg; i < end; ++i) {
                const int t = L.cam_obs[(size_t)i];
                REQUIRE(t >= 0 && t < n_obs && !seen[(size_t)t] && L.cam[(size_t)t] == c, "cam_obs[%d]", i);
                seen[(size_t)t] = 1;
                // ascending inside the chunk and across the camera's chunks
                if (i > 0 && L.cam[(size_t)L.cam_obs[(size_t)i - 1]] == c) REQUIRE(L.cam_obs[(size_t)i - 1] < t, "cam_obs not ascending at %d", i);
            }
            next = end;
        }
        REQUIRE(next == n_obs, "camera chunks do not cover the observations");
        REQUIRE(L.cam_chunk0[0] == 0 && L.cam_chunk0[(size_t)n_real] == (int)nch, "cam_chunk0 ends");
        for (int c = 0; c < n_real; ++c) REQUIRE(L.cam_chunk0[(size_t)c] <= L.cam_chunk0[(size_t)c + 1], "cam_chunk0 decreases at %d", c);
    }

    // ---- Schur tables ----
    const std::vector<int32_t> *const mall[] = {&L.mslot_obs[0], &L.mslot_obs[1], &L.mslot_pc[0], &L.mslot_pc[1], &L.mbatch_slot[0], &L.mbatch_slot[1],
                                                &L.mchunk_batch0[0], &L.mchunk_batch0[1], &L.mchunk_cam0[0], &L.mchunk_cam0[1], &L.slot_obs, &L.chunk_slot,
                                                &L.chunk_cam0, &L.slot_obs_b, &L.chunk_slot_b, &L.chunk_cam0_b, &L.wide_obs};
    if (!schur_tables || n_obs == 0) {
        for (const auto *v : mall) REQUIRE(v->empty(), "a Schur table is not empty without schur_tables");
    } else {
        const int rot = n_real / 2;
        auto idx = [&](int tb, int c) { if (!tb) return c; const int r = c + rot; return r >= n_real ? r - n_real : r; };
        std::vector<Span> span[2] = {std::vector<Span>((size_t)n_pt), std::vector<Span>((size_t)n_pt)};
        for (size_t t = 0; t < no; ++t) for (int tb = 0; tb < 2; ++tb) {
            Span &sp = span[tb][(size_t)L.pt[t]];
            sp.lo = std::min(sp.lo, idx(tb, L.cam[t])); sp.hi = std::max(sp.hi, idx(tb, L.cam[t]));
        }
        std::vector<int> uses(no, 0);
        std::vector<char> in_mf((size_t)n_pt, 0);
        // matrix-core tables (ba_schur_mfma_kernel: a workgroup per chunk, window base cam0; a batch is loaded as <= 64 observations of
        // <= 16 whole points; row of an observation = 6 (index - cam0) + a, index < cam0 + kSchurMfCams "by construction"; the kernel finds
        // "the observation with slot s" of a point by counting the lower bits of its slot mask: slots ascend, none twice)
        for (int tb = 0; tb < 2; ++tb) {
            const auto &so = L.mslot_obs[tb], &pc = L.mslot_pc[tb], &bs = L.mbatch_slot[tb], &cb = L.mchunk_batch0[tb], &c0 = L.mchunk_cam0[tb];
            if (c0.empty()) { REQUIRE(so.empty() && pc.empty() && bs.empty() && cb.empty(), "table %d without chunks is not empty", tb); continue; }
            REQUIRE(cb.size() == c0.size() + 1 && cb[0] == 0 && cb.back() == (int)bs.size() - 1, "mchunk_batch0 of table %d", tb);
            REQUIRE(bs[0] == 0 && bs.back() == (int)so.size() && pc.size() == 2 * so.size(), "mbatch_slot of table %d", tb);
            for (size_t c = 0; c < c0.size(); ++c) {
                REQUIRE(cb[c] < cb[c + 1], "empty chunk %zu in table %d", c, tb);
                for (int b = cb[c]; b < cb[c + 1]; ++b) {
                    REQUIRE(bs[(size_t)b] < bs[(size_t)b + 1] && bs[(size_t)b + 1] - bs[(size_t)b] <= 64, "batch %d of table %d: size", b, tb);
                    int n_points = 0;
                    for (int k = bs[(size_t)b]; k < bs[(size_t)b + 1];) {
                        const int t0 = so[(size_t)k];
                        REQUIRE(t0 >= 0 && t0 < n_obs, "mslot_obs[%d][%d]", tb, k);
                        const int p = L.pt[(size_t)t0], len = pt_len(p);
                        REQUIRE(k + len <= bs[(size_t)b + 1], "point %d is split over batches (table %d)", p, tb);
                        REQUIRE(!in_mf[(size_t)p], "point %d twice in the matrix-core tables", p);
                        in_mf[(size_t)p] = 1; ++n_points;
                        for (int j = 0; j < len; ++j) {
                            const int t = so[(size_t)(k + j)];
                            REQUIRE(t >= 0 && t < n_obs && L.pt[(size_t)t] == p, "slot %d of table %d leaves point %d", k + j, tb, p);
                            uses[(size_t)t]++;
                            const int ci = idx(tb, L.cam[(size_t)t]);
                            REQUIRE(ci >= c0[c] && ci < c0[c] + kSchurMfCams, "camera index %d outside window [%d, +%d) (table %d)", ci, c0[c], kSchurMfCams, tb);
                            if (j) REQUIRE(idx(tb, L.cam[(size_t)so[(size_t)(k + j - 1)]]) < ci, "slots of point %d do not ascend (table %d)", p, tb);
                            REQUIRE(pc[2 * (size_t)(k + j)] == p && pc[2 * (size_t)(k + j) + 1] == L.cam[(size_t)t], "mslot_pc at %d (table %d)", k + j, tb);
                        }
                        k += len;
                    }
                    REQUIRE(n_points <= 16, "batch %d of table %d holds %d points", b, tb, n_points);
                }
            }
        }
        // window tables (ba_schur_window_kernel: a workgroup per chunk walks slots chunk_slot[c] .. chunk_slot[c + 1]; window base
        // chunk_cam0[c]; a camera outside the window goes to global atomics, so "inside the window" is speed, not correctness)
        for (int tb = 0; tb < 2; ++tb) {
            const auto &so = tb ? L.slot_obs_b : L.slot_obs, &cs = tb ? L.chunk_slot_b : L.chunk_slot, &c0 = tb ? L.chunk_cam0_b : L.chunk_cam0;
            if (c0.empty()) { REQUIRE(so.empty() && cs.empty(), "window table %d without chunks is not empty", tb); continue; }
            REQUIRE(cs.size() == c0.size() + 1 && cs[0] == 0 && cs.back() == (int)so.size(), "chunk_slot of table %d", tb);
            int prev_lo = -1;
            for (size_t c = 0; c < c0.size(); ++c) {
                REQUIRE(cs[c] < cs[c + 1], "empty chunk %zu in window table %d", c, tb);
                for (int k = cs[c]; k < cs[c + 1];) {
                    const int t0 = so[(size_t)k];
                    REQUIRE(t0 >= 0 && t0 < n_obs, "slot_obs[%d]", k);
                    const int p = L.pt[(size_t)t0], len = pt_len(p);
                    REQUIRE(k + len <= cs[c + 1], "point %d is split over chunks (window table %d)", p, tb);
                    for (int j = 0; j < len; ++j) {
                        REQUIRE(so[(size_t)(k + j)] == L.pt_start[(size_t)p] + j, "point %d is not whole (window table %d)", p, tb);
                        uses[(size_t)so[(size_t)(k + j)]]++;
                    }
                    REQUIRE(!in_mf[(size_t)p], "point %d is in a matrix-core table too", p);
                    REQUIRE(span[tb][(size_t)p].width() < kSchurWinCams, "point %d spans %d cameras (window table %d)", p, span[tb][(size_t)p].width(), tb);
                    REQUIRE(span[tb][(size_t)p].lo >= prev_lo, "points not ordered by lowest camera at %d (window table %d)", p, tb);
                    if (k == cs[c]) REQUIRE(c0[c] == span[tb][(size_t)p].lo, "chunk_cam0[%zu] of window table %d", c, tb);
                    prev_lo = span[tb][(size_t)p].lo;
                    k += len;
                }
            }
        }
        // wide list (ba_schur_kernel over wide_obs): the rest
        std::vector<char> want_wide(no, 0);
        for (int p = 0; p < n_pt; ++p)
            if (pt_len(p) > 0 && !in_mf[(size_t)p] && span[0][(size_t)p].width() >= kSchurWinCams && span[1][(size_t)p].width() >= kSchurWinCams)
                for (int t = L.pt_start[(size_t)p]; t < L.pt_start[(size_t)p + 1]; ++t) want_wide[(size_t)t] = 1;
        size_t n_want = 0;
        for (size_t t = 0; t < no; ++t) n_want += want_wide[t];
        REQUIRE(L.wide_obs.size() == n_want, "wide_obs holds %zu observations, expected %zu", L.wide_obs.size(), n_want);
        for (int t : L.wide_obs) { REQUIRE(t >= 0 && t < n_obs && want_wide[(size_t)t], "observation %d does not belong in wide_obs", t); uses[(size_t)t]++; }
        for (size_t t = 0; t < no; ++t) REQUIRE(uses[t] == 1, "observation %zu appears %d times across the Schur tables", t, uses[t]);
    }

    // ---- point chunks (ba_backsub_chunk_kernel / ba_point_prep_chunk_kernel: a workgroup of kPtChunkObs threads per chunk, one
    // thread per observation and per point in LDS arrays of kPtChunkObs rows; a chunk with more observations must be one point) ----
    {
        const size_t n = L.pchunk_pt0.size() - 1;
        REQUIRE(!L.pchunk_pt0.empty() && L.pchunk_pt0[0] == 0 && L.pchunk_pt0.back() == n_pt, "pchunk_pt0 ends");
        REQUIRE(L.pchunk_info.size() == 4 * std::max<size_t>(n, 1), "pchunk_info size");
        for (size_t c = 0; c < n; ++c) {
            const int p0 = L.pchunk_pt0[c], p1 = L.pchunk_pt0[c + 1];
            REQUIRE(p0 < p1 && p1 - p0 <= kPtChunkObs, "point chunk %zu: %d points", c, p1 - p0);
            const int nobs = L.pt_start[(size_t)p1] - L.pt_start[(size_t)p0];
            REQUIRE(nobs <= kPtChunkObs || p1 - p0 == 1, "point chunk %zu: %d observations over %d points", c, nobs, p1 - p0);
            REQUIRE(L.pchunk_info[4 * c] == p0 && L.pchunk_info[4 * c + 1] == p1 && L.pchunk_info[4 * c + 2] == L.pt_start[(size_t)p0] &&
                    L.pchunk_info[4 * c + 3] == L.pt_start[(size_t)p1], "pchunk_info[%zu]", c);
        }
    }
}

// which table families a scene with Schur tables fills: the inputs below must reach every branch
struct Filled { bool mf[2], win[2], wide; };
Filled filled(const Scene &s, int num_cu)
{
    const BaLayout L = make_ba_layout(s.n_real, s.n_pt, (int)s.cam.size(), s.cam.data(), s.pt.data(), num_cu, true);
    return {{!L.mchunk_cam0[0].empty(), !L.mchunk_cam0[1].empty()}, {!L.chunk_cam0.empty(), !L.chunk_cam0_b.empty()}, !L.wide_obs.empty()};
}

}  // namespace

int main()
{
    std::vector<std::pair<std::string, Scene>> scenes;
    auto fixed = [](int n) { return [n](int, std::mt19937 &) { return n; }; };
    // closed camera loops as synth.ba_scene makes them: ten consecutive cameras per point; the seam fills table 1
    for (int n_real : {33, 96, 200, 512}) scenes.push_back({"ring" + std::to_string(n_real), ring(n_real, 40 * n_real, 100u + (unsigned)n_real, fixed(10))});
    // tracks of 14 to 27 cameras: too long for the matrix-core tables, narrow enough for the windows (and their seam)
    scenes.push_back({"window96", ring(96, 3000, 5, [](int, std::mt19937 &r) { return 14 + (int)(r() % 14u); }, false)});
    // tracks spanning more than 28 cameras in both index spaces, among short ones
    // (28 cameras: the widest window track; 29: the narrowest wide one)
    scenes.push_back({"wide36", ring(36, 1500, 6, [](int p, std::mt19937 &r) { return p % 3 ? 4 + (int)(r() % 6u) : 28 + (int)(r() % 7u); })});
    // tracks of two or three cameras: a matrix-core batch fills its 16 points before its 64 observations
    scenes.push_back({"short64", ring(64, 4000, 10, [](int, std::mt19937 &r) { return 2 + (int)(r() % 2u); })});
    {   // a point observed twice by one camera, points without observations, one track longer than 256
        Scene s = ring(40, 2000, 7, [](int p, std::mt19937 &) { return p % 11 == 4 ? 0 : 6; }, false);
        for (int p : {0, 17, 900}) { s.cam.push_back(s.cam[(size_t)(std::find(s.pt.begin(), s.pt.end(), p) - s.pt.begin())]); s.pt.push_back(p); }
        for (int j = 0; j < 300; ++j) { s.cam.push_back(j % 40); s.pt.push_back(4); }
        scenes.push_back({"odd40", s});
    }
    bool mf[2] = {false, false}, win[2] = {false, false}, wide = false;
    for (const auto &sc : scenes) for (int num_cu : {256, 1}) {
        g_case = sc.first + "/cu" + std::to_string(num_cu);
        check(sc.second, num_cu, true);
        const Filled f = filled(sc.second, num_cu);
        for (int tb = 0; tb < 2; ++tb) { mf[tb] |= f.mf[tb]; win[tb] |= f.win[tb]; }
        wide |= f.wide;
    }
    if (!(mf[0] && mf[1] && win[0] && win[1] && wide)) { printf("FAIL the scenes do not fill every table: mf %d %d win %d %d wide %d\n", mf[0], mf[1], win[0], win[1], wide); ++g_failed; }
    // without Schur tables: 32 cameras or fewer (the LDS-slab form), no observations, no cameras
    for (int num_cu : {256, 1}) {
        g_case = "ring25/off"; check(ring(25, 1000, 8, fixed(4)), num_cu, false);
        g_case = "ring32/off"; check(ring(32, 1500, 9, fixed(12)), num_cu, false);
        Scene empty; empty.n_real = 40; empty.n_pt = 300;
        g_case = "n_obs0/on"; check(empty, num_cu, true);
        g_case = "n_obs0/off"; check(empty, num_cu, false);
        Scene none; none.n_pt = 7;
        g_case = "n_real0"; check(none, num_cu, true);
        Scene nothing;
        g_case = "nothing"; check(nothing, num_cu, false);
    }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("ba layout ok: %zu scenes\n", scenes.size());
    return 0;
}
