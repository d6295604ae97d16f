// Index tables of one bundle-adjustment problem: see ba_layout.hpp.
#include "ba_layout.hpp"

#include <algorithm>
#include <climits>
#include <cstddef>

namespace esfm {

BaPointSort ba_sort_by_point(int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx)
{
    BaPointSort s;
    s.pt_start.assign((size_t)n_pt + 1, 0);
    s.order.resize((size_t)n_obs); s.cam.resize((size_t)n_obs); s.pt.resize((size_t)n_obs);
    for (int k = 0; k < n_obs; ++k) s.pt_start[(size_t)pt_idx[k] + 1]++;
    for (int p = 0; p < n_pt; ++p) s.pt_start[(size_t)p + 1] += s.pt_start[(size_t)p];
    std::vector<int32_t> fill(s.pt_start.begin(), s.pt_start.end() - 1);
    for (int k = 0; k < n_obs; ++k) {
        const size_t t = (size_t)fill[(size_t)pt_idx[k]]++;
        s.order[t] = k; s.cam[t] = cam_idx[k]; s.pt[t] = pt_idx[k];
    }
    return s;
}

namespace {

// camera CSR of the (point-sorted) observations, cut into chunks, for the atomic-free per-camera sums
void build_camera_chunks(BaLayout &L, int n_real)
{
    const int n_obs = (int)L.cam.size();
    std::vector<int32_t> cstart((size_t)n_real + 1, 0);
    for (int t = 0; t < n_obs; ++t) cstart[(size_t)L.cam[(size_t)t] + 1]++;
    L.cam_nobs.assign(cstart.begin() + 1, cstart.end());
    for (int c = 0; c < n_real; ++c) cstart[(size_t)c + 1] += cstart[(size_t)c];
    L.cam_obs.resize((size_t)n_obs);
    std::vector<int32_t> fill(cstart.begin(), cstart.end() - 1);
    for (int t = 0; t < n_obs; ++t) L.cam_obs[(size_t)fill[(size_t)L.cam[(size_t)t]]++] = t;
    L.cam_chunk0.assign((size_t)n_real + 1, 0);
    for (int c = 0; c < n_real; ++c) {
        L.cam_chunk0[(size_t)c] = (int32_t)L.cchunk_cam.size();
        for (int b0 = cstart[(size_t)c]; b0 < cstart[(size_t)c + 1]; b0 += kCamChunk) {
            L.cchunk_cam.push_back(c); L.cchunk_beg.push_back(b0); L.cchunk_end.push_back(std::min(b0 + kCamChunk, cstart[(size_t)c + 1]));
        }
    }
    L.cam_chunk0[(size_t)n_real] = (int32_t)L.cchunk_cam.size();
}

// lowest / highest camera of every point, in the plain [0] and the rotated [1] index space
struct CamSpan {
    int n_real, rot;
    std::vector<int32_t> lo[2], hi[2];
    int rotated(int c) const { const int r = c + rot; return r >= n_real ? r - n_real : r; }
    int width(int tb, int p) const { return hi[tb][(size_t)p] - lo[tb][(size_t)p]; }
};

// The matrix-core tables, cut into chunks of `per` observations (a chunk also ends where a point's cameras would leave the window of
// kSchurMfCams indices behind the chunk's first); returns the number of chunks of both tables (= workgroups of the one launch).
// record: write the lists (into the empty tables) -- else only count.
int64_t walk_mf_chunks(BaLayout &L, const CamSpan &sp, const std::vector<int32_t> (&mperm)[2], int64_t per, bool record)
{
    int64_t n_chunks = 0;
    for (int tb = 0; tb < 2; ++tb) {
        std::vector<int32_t> &slot_obs = L.mslot_obs[tb], &batch_slot = L.mbatch_slot[tb];
        int64_t in_chunk = 0, n_tb = 0; int cw = 0, in_batch = 0, pts_batch = 0;
        for (int p : mperm[tb]) {
            const int t = L.pt_start[(size_t)p + 1] - L.pt_start[(size_t)p];
            const bool new_chunk = n_tb == 0 || in_chunk >= per || sp.hi[tb][(size_t)p] - cw >= kSchurMfCams;
            if (new_chunk) { ++n_tb; cw = sp.lo[tb][(size_t)p]; in_chunk = 0; }
            in_chunk += t;
            if (!record) continue;
            if (new_chunk) { L.mchunk_batch0[tb].push_back((int32_t)batch_slot.size()); L.mchunk_cam0[tb].push_back(cw); }
            if (new_chunk || in_batch + t > 64 || pts_batch >= 16) { batch_slot.push_back((int32_t)slot_obs.size()); in_batch = 0; pts_batch = 0; }
            // a point's observations in ascending camera-slot order (the kernel finds "the observation with slot s" by counting
            // the lower bits of the point's slot mask); in the seam's table that is the ROTATED index
            const size_t at = slot_obs.size();
            for (int k = L.pt_start[(size_t)p]; k < L.pt_start[(size_t)p + 1]; ++k) slot_obs.push_back(k);
            std::sort(slot_obs.begin() + (std::ptrdiff_t)at, slot_obs.end(), [&](int32_t a, int32_t b) {
                const int ca = tb ? sp.rotated(L.cam[(size_t)a]) : L.cam[(size_t)a], cb = tb ? sp.rotated(L.cam[(size_t)b]) : L.cam[(size_t)b];
                return ca < cb;
            });
            in_batch += t; ++pts_batch;
        }
        if (record && n_tb > 0) {
            batch_slot.push_back((int32_t)slot_obs.size());
            L.mchunk_batch0[tb].push_back((int32_t)batch_slot.size() - 1);
        }
        n_chunks += n_tb;
    }
    return n_chunks;
}

// one windowed table: the points of `perm` by lowest camera, the observation stream cut into ~2 chunks per CU
void build_window_table(const BaLayout &L, std::vector<int32_t> &perm, const std::vector<int32_t> &lo, int num_cu, std::vector<int32_t> &slots,
                        std::vector<int32_t> &cslot, std::vector<int32_t> &ccam0)
{
    if (perm.empty()) return;
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return lo[(size_t)a] < lo[(size_t)b]; });
    int64_t total = 0;
    for (int p : perm) total += L.pt_start[(size_t)p + 1] - L.pt_start[(size_t)p];
    const int want_chunks = std::max(1, 2 * num_cu);     // (1 to 6 chunks per CU measured alike on BA-512: 0.85-0.89 ms)
    const int64_t per = std::max<int64_t>(1024, (total + want_chunks - 1) / want_chunks);
    slots.reserve((size_t)total);
    int64_t in_chunk = 0;
    for (int p : perm) {
        if (cslot.empty() || in_chunk >= per) { cslot.push_back((int32_t)slots.size()); ccam0.push_back(lo[(size_t)p]); in_chunk = 0; }
        for (int t = L.pt_start[(size_t)p]; t < L.pt_start[(size_t)p + 1]; ++t) slots.push_back(t);
        in_chunk += L.pt_start[(size_t)p + 1] - L.pt_start[(size_t)p];
    }
    cslot.push_back((int32_t)slots.size());
}

// Schur complement of large camera counts.  Narrow tracks -- at most kSchurMfCams camera indices wide, no camera twice -- take the
// matrix-core kernel: per point the Schur update is the rank-3 product (W M^-1) W' over its cameras' rows, a small dense GEMM once
// points with the same cameras are processed together.  The others go to the windowed kernel: points ordered by their lowest camera,
// the observation stream cut into chunks.  Either kind has a second table, on camera indices rotated by half the camera count, for
// the tracks that are only narrow there (the seam of a closed camera loop); what is wide in both index spaces goes to the plain kernel.
void build_schur_tables(BaLayout &L, int n_real, int n_pt, int num_cu)
{
    const int n_obs = (int)L.cam.size();
    CamSpan sp;
    sp.n_real = n_real; sp.rot = n_real / 2;
    for (int tb = 0; tb < 2; ++tb) { sp.lo[tb].assign((size_t)n_pt, INT32_MAX); sp.hi[tb].assign((size_t)n_pt, -1); }
    for (int t = 0; t < n_obs; ++t) {
        const size_t p = (size_t)L.pt[(size_t)t];
        const int c = L.cam[(size_t)t], cr = sp.rotated(c);
        sp.lo[0][p] = std::min(sp.lo[0][p], c); sp.hi[0][p] = std::max(sp.hi[0][p], c);
        sp.lo[1][p] = std::min(sp.lo[1][p], cr); sp.hi[1][p] = std::max(sp.hi[1][p], cr);
    }
    std::vector<int32_t> mperm[2];
    std::vector<char> taken((size_t)n_pt, 0);
    for (int p = 0; p < n_pt; ++p) {
        const int b = L.pt_start[(size_t)p], e = L.pt_start[(size_t)p + 1];
        if (e <= b || e - b > kSchurMfCams) continue;
        bool dup = false;
        for (int t = b; t < e && !dup; ++t) for (int u = b; u < t; ++u) if (L.cam[(size_t)t] == L.cam[(size_t)u]) { dup = true; break; }
        if (dup) continue;
        if (sp.width(0, p) < kSchurMfCams) { mperm[0].push_back(p); taken[(size_t)p] = 1; }
        else if (sp.width(1, p) < kSchurMfCams) { mperm[1].push_back(p); taken[(size_t)p] = 1; }
    }
    int64_t total_all = 0;
    for (int tb = 0; tb < 2; ++tb) {
        const std::vector<int32_t> &lo = sp.lo[tb];
        std::stable_sort(mperm[tb].begin(), mperm[tb].end(), [&](int a, int b) { return lo[(size_t)a] < lo[(size_t)b]; });
        for (int p : mperm[tb]) total_all += L.pt_start[(size_t)p + 1] - L.pt_start[(size_t)p];
    }
    // Both tables run in ONE launch of two workgroups per CU (ba_schur_mfma_kernel: 78 KB of LDS, 244 registers): every chunk should
    // be resident from the start -- a chunk dispatched behind the others adds its whole length to the launch (round 5: the seam's
    // table had its own, much smaller `per`: a hundred short chunks behind 512 long ones, 20 us of tail).  One `per` for both, raised
    // by 1 % until the chunks fit the slots; camera windows can force more chunks than that (wide, scattered tracks): then the
    // first `per` stands.
    {
        const int64_t slots = 2 * (int64_t)std::max(1, num_cu);
        const int64_t per0 = std::max<int64_t>(512, (total_all + slots - 1) / slots);
        int64_t per = per0;
        bool fits = false;
        for (int it = 0; it < 64 && !fits; ++it) {
            fits = walk_mf_chunks(L, sp, mperm, per, false) <= slots;
            if (!fits) per += std::max<int64_t>(1, per / 100);
        }
        walk_mf_chunks(L, sp, mperm, fits ? per : per0, true);
    }
    for (int tb = 0; tb < 2; ++tb) {
        L.mslot_pc[tb].resize(2 * L.mslot_obs[tb].size());
        for (size_t k = 0; k < L.mslot_obs[tb].size(); ++k) {
            L.mslot_pc[tb][2 * k] = L.pt[(size_t)L.mslot_obs[tb][k]]; L.mslot_pc[tb][2 * k + 1] = L.cam[(size_t)L.mslot_obs[tb][k]];
        }
    }
    std::vector<int32_t> perm_a, perm_b;
    for (int p = 0; p < n_pt; ++p) {
        if (L.pt_start[(size_t)p + 1] <= L.pt_start[(size_t)p] || taken[(size_t)p]) continue;
        if (sp.width(0, p) < kSchurWinCams) perm_a.push_back(p);
        else if (sp.width(1, p) < kSchurWinCams) perm_b.push_back(p);
        else for (int t = L.pt_start[(size_t)p]; t < L.pt_start[(size_t)p + 1]; ++t) L.wide_obs.push_back(t);
    }
    build_window_table(L, perm_a, sp.lo[0], num_cu, L.slot_obs, L.chunk_slot, L.chunk_cam0);
    build_window_table(L, perm_b, sp.lo[1], num_cu, L.slot_obs_b, L.chunk_slot_b, L.chunk_cam0_b);
}

void build_point_chunks(BaLayout &L, int n_pt)
{
    int p = 0;
    while (p < n_pt) {
        L.pchunk_pt0.push_back(p);
        int obs = 0, pts_in = 0;
        while (p < n_pt && pts_in < kPtChunkObs) {
            const int t = L.pt_start[(size_t)p + 1] - L.pt_start[(size_t)p];
            if (pts_in > 0 && obs + t > kPtChunkObs) break;
            obs += t; ++pts_in; ++p;
            if (obs > kPtChunkObs) break;       // a single long track
        }
    }
    L.pchunk_pt0.push_back(n_pt);
    const size_t n_pchunks = L.pchunk_pt0.size() - 1;
    L.pchunk_info.assign(4 * std::max<size_t>(n_pchunks, 1), 0);
    for (size_t c = 0; c < n_pchunks; ++c) {
        const int p0 = L.pchunk_pt0[c], p1 = L.pchunk_pt0[c + 1];
        L.pchunk_info[4 * c] = p0; L.pchunk_info[4 * c + 1] = p1;
        L.pchunk_info[4 * c + 2] = L.pt_start[(size_t)p0]; L.pchunk_info[4 * c + 3] = L.pt_start[(size_t)p1];
    }
}

}  // namespace

BaLayout make_ba_layout(int n_real, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, int num_cu, bool schur_tables)
{
    BaLayout L;
    static_cast<BaPointSort &>(L) = ba_sort_by_point(n_pt, n_obs, cam_idx, pt_idx);
    build_camera_chunks(L, n_real);
    if (schur_tables && n_obs > 0) build_schur_tables(L, n_real, n_pt, num_cu);
    build_point_chunks(L, n_pt);
    return L;
}

}  // namespace esfm
