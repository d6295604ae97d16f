// Stand-alone host driver of ransac_host.hpp's registrator replay (no GPU call is made): fill_round / replay_round over rounds whose
// model counts and inlier counts come from a table on stdin instead of from kernels.  tests/test_ransac_rounds_cpu.py writes the table,
// computes what a one-iteration-at-a-time loop reaches and compares; built there once plainly and once with
// -fsanitize=address,undefined.
//
// stdin:  model_points models_per_slot max_iters chunk confidence n_pairs, then per pair: count fail_at n_rows and n_rows rows
//         "n_models c_0 .. c_{n_models - 1}" -- row i is what iteration i of that pair yields (iterations past the table: no model).
//         model_points 5 draws the plain 5-subset (fail_at is not looked at); 4 draws the 4-subset with the subset check on the points
//         (i, i * i) -> (i, +- i * i), minus where i % 3 == 2, so that some subsets are rejected for their orientation; the pair's draw
//         number fail_at (none if < 0) sees the collinear points (i, i) in the first image instead and gives up.
// stdout: per round and pair "fill round pair valid idle_slots rng_state idx.." (the indices of the valid slots),
//         per new best "take round pair iteration model", at the end "rounds R" and per pair
//         "result pair best_iteration best_model max_good iter niters done failed".
// Idle slots, and the counts behind a slot's n_models, hold a winning count: a replay that reads one of them prints a wrong result.
#include <cstdio>
#include <vector>

#include "../../easysfm_amd/csrc/ransac_host.hpp"

using namespace esfm::ransac;

struct Problem {
    int count = 0, fail_at = -1, draws = 0;
    std::vector<std::vector<int>> rows;
    std::vector<float> curve, line, image2;
    int best_iter = -1, best_model = -1;
};

int main()
{
    int model_points, models_per_slot, max_iters, chunk, n_pairs;
    double confidence;
    if (std::scanf("%d %d %d %d %lf %d", &model_points, &models_per_slot, &max_iters, &chunk, &confidence, &n_pairs) != 6) return 2;
    if ((model_points != kFivePoints && model_points != kFourPoints) || models_per_slot < 1 || chunk < 1 || n_pairs < 0) return 2;
    std::vector<Problem> P((size_t)n_pairs);
    std::vector<Registrator> S;
    std::vector<int32_t> off(1, 0);
    for (Problem &q : P) {
        int n_rows;
        if (std::scanf("%d %d %d", &q.count, &q.fail_at, &n_rows) != 3 || q.count < 0 || n_rows < 0) return 2;
        q.rows.resize((size_t)n_rows);
        for (std::vector<int> &row : q.rows) {
            int nm;
            if (std::scanf("%d", &nm) != 1 || nm < 0 || nm > models_per_slot) return 2;
            row.resize((size_t)nm);
            for (int &c : row) if (std::scanf("%d", &c) != 1) return 2;
        }
        for (int i = 0; i < q.count; ++i) { q.curve.push_back((float)i); q.curve.push_back((float)(i * i)); q.line.push_back((float)i); q.line.push_back((float)i);
                                            q.image2.push_back((float)i); q.image2.push_back((float)(i % 3 == 2 ? -i * i : i * i)); }
        off.push_back(off.back() + q.count);
        S.emplace_back(model_points, max_iters, q.count);
    }
    const RoundTables T(n_pairs, chunk, model_points, models_per_slot);
    std::vector<int32_t> tab(T.end, -12345);
    const auto draw = [&](int p) {
        return [q = &P[(size_t)p], model_points](CvRng &rng, int32_t *idx) {
            if (model_points == kFivePoints) { draw_subset(rng, q->count, idx); return true; }
            return draw_subset(rng, q->count, q->draws++ == q->fail_at ? q->line.data() : q->curve.data(), q->image2.data(), idx);
        };
    };
    int round = 0;
    for (; fill_round(S.data(), n_pairs, chunk, tab.data() + T.samples, draw); ++round) {
        std::vector<int> start((size_t)n_pairs);
        for (int p = 0; p < n_pairs; ++p) {
            const Problem &q = P[(size_t)p];
            const Registrator &s = S[(size_t)p];
            start[(size_t)p] = s.iter;
            int idle = 0;
            for (int k = 0; k < chunk; ++k) {
                const size_t g = (size_t)chunk * p + k;
                const bool is_idle = tab[T.samples + (size_t)model_points * g] < 0;
                const size_t row = (size_t)(s.iter + k);
                const int nm = is_idle ? models_per_slot : (row < q.rows.size() ? (int)q.rows[row].size() : 0);
                idle += is_idle ? 1 : 0;
                tab[T.n_models + g] = nm;
                for (int m = 0; m < models_per_slot; ++m) tab[T.counts + (size_t)models_per_slot * g + m] = !is_idle && m < nm ? q.rows[row][(size_t)m] : q.count;
            }
            std::printf("fill %d %d %d %d %llu", round, p, s.valid, idle, (unsigned long long)s.rng.state);
            for (int k = 0; k < model_points * s.valid; ++k) std::printf(" %d", tab[T.samples + (size_t)model_points * chunk * p + k]);
            std::printf("\n");
        }
        const int n_take = replay_round(S.data(), n_pairs, off.data(), chunk, tab.data() + T.n_models, tab.data() + T.counts, models_per_slot, confidence,
                                        tab.data() + T.take);
        for (int e = 0; e < n_take; ++e) {
            const int32_t *t = &tab[T.take + 3 * (size_t)e];
            Problem &q = P[(size_t)t[0]];
            q.best_iter = start[(size_t)t[0]] + (t[1] - chunk * t[0]); q.best_model = t[2];
            std::printf("take %d %d %d %d\n", round, t[0], q.best_iter, q.best_model);
        }
    }
    std::printf("rounds %d\n", round);
    for (int p = 0; p < n_pairs; ++p) {
        const Registrator &s = S[(size_t)p];
        std::printf("result %d %d %d %d %d %d %d %d\n", p, P[(size_t)p].best_iter, P[(size_t)p].best_model, s.max_good, s.iter, s.niters, s.done ? 1 : 0, s.failed ? 1 : 0);
    }
    return 0;
}
