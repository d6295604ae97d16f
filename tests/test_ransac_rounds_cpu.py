"""The registrator replay of easysfm_amd/csrc/ransac_host.hpp (Registrator, fill_round, replay_round) without a GPU: tests/cpp/
ransac_rounds_check_main.cpp drives it over rounds whose model and inlier counts come from a table, and this file compares what it
prints with a plain one-iteration-at-a-time loop written here on homography_ref's CvRng and update_num_iters -- the loop
RANSACPointSetRegistrator::run is.  The promise under test: the outcome does not depend on the chunk size, and the generator stands
after every round where that loop has it.  The program is built once plainly and once with -fsanitize=address,undefined; every table
goes through both."""
import os
import subprocess

import numpy as np
import pytest

import homography_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (1, 3, 63, 64, 65, 1024)
MODELS = {"essential": (5, 10, 1000, 0.99), "homography": (4, 1, 2000, 0.995)}   # model points, models per slot, max iterations, confidence


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("ransac_rounds")
    out = []
    for name, flags in (("plain", ["-O2"]), ("asan_ubsan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / name)
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", *flags, os.path.join(ROOT, "tests", "cpp", "ransac_rounds_check_main.cpp"),
                            "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        out.append(exe)
    return out


# ---- the sequential loop ----------------------------------------------------------------------------------------------------------
def _points(count):
    """the program's point sets: image 1, image 2 (orientation flipped where i % 3 == 2), and the collinear set of a failing draw"""
    return ([[float(i), float(i * i)] for i in range(count)], [[float(i), float(-i * i if i % 3 == 2 else i * i)] for i in range(count)],
            [[float(i), float(i)] for i in range(count)])


class Sequential:
    """One problem, one iteration at a time.  draws[k] = (indices or None, generator state after draw k); niters_at[i] = niters when
    iteration i begins (and, at i = iter, when the loop ended)."""

    def __init__(self, model, count, rows, fail_at=-1):
        self.mp, self.mps, self.max_iters, self.conf = MODELS[model]
        self.count, self.rows, self.fail_at = count, rows, fail_at
        self.rng, self.draws, self.pts = R.CvRng(), [], _points(count)
        self.best, self.max_good, self.iter, self.niters, self.failed, self.niters_at = (-1, -1), 0, 0, self.max_iters, False, []
        self.exact = count == self.mp
        if count < self.mp:
            return
        if self.exact:
            if rows and len(rows[0]) > 0:
                self.best, self.max_good = (0, 0), count
            return
        while self.iter < self.niters:
            self.niters_at.append(self.niters)
            self.draw_upto(self.iter + 1)
            if self.draws[self.iter][0] is None:
                self.failed = True
                break
            for m, good in enumerate(rows[self.iter] if self.iter < len(rows) else []):
                if good > max(self.max_good, self.mp - 1):
                    self.best, self.max_good = (self.iter, m), good
                    self.niters = R.update_num_iters(self.conf, (count - good) / count, self.mp, self.niters)
            self.iter += 1
        self.niters_at.append(self.niters)

    def draw_upto(self, n):
        """the stream, continued past the loop's end where a chunk draws ahead of it; it stops at a draw that gives up"""
        while len(self.draws) < n and not (self.draws and self.draws[-1][0] is None):
            if self.mp == 5:
                idx = []
                while len(idx) < 5:
                    v = self.rng.uniform(0, self.count)
                    if v not in idx:
                        idx.append(v)
            else:
                idx = R.draw_subset(self.rng, self.count, self.pts[2] if len(self.draws) == self.fail_at else self.pts[0], self.pts[1])
            self.draws.append((idx, self.rng.state))

    def result(self):
        return (*self.best, self.max_good, self.iter, self.niters, 1, int(self.failed))

    def rounds(self, chunk):
        """what fill_round must do round by round: [(valid, indices of the valid slots, generator state afterwards)]"""
        if self.count < self.mp:
            return []
        if self.exact:
            return [(1, list(range(self.mp)), R.CvRng().state)]
        out, it = [], 0
        while True:
            valid = min(chunk, self.niters_at[it] - it)            # the rule: no more draws than the loop can still use
            self.draw_upto(it + valid)
            gave_up = len(self.draws) <= it + valid and self.draws[-1][0] is None
            if gave_up:
                valid = len(self.draws) - 1 - it
            flat = [v for idx, _ in self.draws[it:it + valid] for v in idx]
            out.append((valid, flat, self.draws[it + valid - 1 + (1 if gave_up else 0)][1] if self.draws else R.CvRng().state))
            it = min(it + valid, self.iter)
            if gave_up or it >= self.niters_at[it]:
                return out


# ---- the program ------------------------------------------------------------------------------------------------------------------
def _run(programs, model, chunk, problems):
    mp, mps, max_iters, conf = MODELS[model]
    text = [f"{mp} {mps} {max_iters} {chunk} {conf!r} {len(problems)}"]
    for count, rows, fail_at in problems:
        text.append(f"{count} {fail_at} {len(rows)}")
        text.extend(" ".join(str(v) for v in [len(r), *r]) for r in rows)
    outs = [subprocess.run([exe], input="\n".join(text) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for exe in programs]
    for r in outs:
        assert r.returncode == 0, r.stdout[-4000:]
    assert outs[0].stdout == outs[1].stdout
    fills, takes, results, n_rounds = [[] for _ in problems], [[] for _ in problems], {}, None
    for line in outs[0].stdout.splitlines():
        kind, *v = line.split()
        v = [int(x) for x in v]
        if kind == "fill":
            assert v[0] == len(fills[v[1]])
            fills[v[1]].append((v[2], v[3], v[4], v[5:]))
        elif kind == "take":
            takes[v[1]].append((v[2], v[3]))
        elif kind == "rounds":
            n_rounds = v[0]
        else:
            assert kind == "result"
            results[v[0]] = tuple(v[1:])
    return fills, takes, results, n_rounds


def check(programs, model, chunk, problems):
    """every problem of the batch against its own sequential loop; -> the Sequential objects"""
    mp = MODELS[model][0]
    seqs = [Sequential(model, count, rows, fail_at) for count, rows, fail_at in problems]
    # rows the loop never reaches win everything if a replay reads them (the program does the same for idle slots)
    poisoned = []
    for s, (count, rows, fail_at) in zip(seqs, problems):
        rows = [list(r) for r in rows] + [[] for _ in range(max(0, s.iter + 3 - len(rows)))]
        if not s.exact and count >= mp:
            for i in range(s.iter, s.iter + 3):
                rows[i] = [count] * MODELS[model][1]
        poisoned.append((count, rows, fail_at))
    fills, takes, results, n_rounds = _run(programs, model, chunk, poisoned)
    want_rounds = [s.rounds(chunk) for s in seqs]
    assert n_rounds == max(len(w) for w in want_rounds)
    for p, (s, want) in enumerate(zip(seqs, want_rounds)):
        assert results[p] == s.result(), (model, chunk, p)
        assert len(fills[p]) == n_rounds
        state = R.CvRng().state
        for r, (valid, idle, got_state, idx) in enumerate(fills[p]):
            if r < len(want):
                assert (valid, idx, got_state) == want[r], (model, chunk, p, r)
                state = got_state
            else:                                                   # a finished pair: idle slots only, the generator at rest
                assert (valid, idx, got_state) == (0, [], state), (model, chunk, p, r)
            assert idle == chunk - valid
        assert (takes[p][-1] if takes[p] else (-1, -1)) == s.best
    return seqs


def _noise(seed, n_iter, mps, hi):
    rng = np.random.default_rng(seed)
    return [[int(c) for c in rng.integers(0, hi, int(rng.integers(0, mps + 1)))] for _ in range(n_iter)]


def _planted(model, seed, plants, n_iter=300, count=200, hi=12):
    """model counts 0 .. models_per_slot and inlier counts below hi per iteration from a seeded stream, `plants` = {iteration: count}
    written into that iteration's last model"""
    rows = _noise(seed, n_iter, MODELS[model][1], hi)
    for i, good in plants.items():
        rows[i] = (rows[i] or [0])[:-1] + [good]
    return (count, rows, -1)


def _good_for(model, count, niters):
    """an inlier count after which update_num_iters gives exactly `niters`"""
    mp, _, max_iters, conf = MODELS[model]
    return next(g for g in range(count, mp - 1, -1) if R.update_num_iters(conf, (count - g) / count, mp, max_iters) == niters)


SCENARIOS = {
    "first_slot": {128: 100},                 # first slot of the third round of 64; iteration 0 would be every chunk's
    "first_of_all": {0: 100},
    "middle_slot": {31: 100},
    "last_slot": {63: 60, 64: 100, 129: 120},  # last of 64's first round, last of 65's first and second
    "never": None,
}


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("model", MODELS)
def test_chunk_size_independence(programs, model, scenario):
    """one fixed stream of model counts and inlier counts; chunk 1, 3, 63, 64, 65 and 1024 all reach the sequential loop's (best
    iteration, best model, max_good, iter, niters)"""
    mp, mps, max_iters, _ = MODELS[model]
    problem = _planted(model, 7, SCENARIOS[scenario]) if SCENARIOS[scenario] else (200, _noise(7, max_iters, mps, mp), -1)
    for chunk in CHUNKS:
        s, = check(programs, model, chunk, [problem])
    if scenario == "never":
        assert s.result() == (-1, -1, 0, max_iters, max_iters, 1, 0)
    else:
        assert s.best[0] in SCENARIOS[scenario] and s.iter < max_iters


@pytest.mark.parametrize("model", MODELS)
def test_niters_shrinks_inside_a_chunk(programs, model):
    """the best model at iteration 10 cuts niters to 17: the slots from 17 on, which hold winning counts, are not counted"""
    problem = _planted(model, 3, {10: _good_for(model, 200, 17)}, hi=MODELS[model][0])
    for chunk in (64, 1024):
        s, = check(programs, model, chunk, [problem])
        assert s.result()[:5] == (10, len(problem[1][10]) - 1, _good_for(model, 200, 17), 17, 17)


@pytest.mark.parametrize("at", [0, 2])
@pytest.mark.parametrize("model", MODELS)
def test_niters_reaches_iter_at_a_chunk_boundary(programs, model, at):
    """niters falls to 3 inside a round of 3: the pair ends with the round and no further round is filled"""
    problem = _planted(model, 4, {at: _good_for(model, 100, 3)}, count=100, hi=MODELS[model][0])
    s, = check(programs, model, 3, [problem])
    assert s.result()[3:5] == (3, 3) and len(s.rounds(3)) == 1
    s, = check(programs, model, 1, [problem])
    assert len(s.rounds(1)) == 3


def test_valid_rule_and_the_five_point_stream(programs):
    """a pair that runs three rounds of 64 draws 64, 64 and min(64, niters - iter) = 17 samples -- the generator state after each
    round is checked in check() -- and they are the first 145 samples of esfm_ransac_sample_stream"""
    from easysfm_amd import motion
    good = _good_for("essential", 200, 145)
    problem = _planted("essential", 5, {40: good}, hi=5)
    s, = check(programs, "essential", 64, [problem])
    assert [v for v, _, _ in s.rounds(64)] == [64, 64, 17] and s.iter == 145
    fills = _run(programs, "essential", 64, [problem])[0][0]
    got = np.array([v for f in fills for v in f[3]], np.int32).reshape(-1, 5)
    assert np.array_equal(got, motion.ransac_sample_stream(200, 145))
    # chunk 1024 draws 1000 in its only round: the stream is the same, the loop uses its first 145
    assert [v for v, _, _ in s.rounds(1024)] == [1000]


@pytest.mark.parametrize("model", MODELS)
def test_exactly_model_points(programs, model):
    """count == model points: one slot with the indices 0 .. m - 1, no iteration; max_good = count if the slot has a model"""
    mp, mps = MODELS[model][:2]
    for chunk in (1, 64):
        s, = check(programs, model, chunk, [(mp, [[3] * mps], -1)])
        assert s.result() == (0, 0, mp, 0, MODELS[model][2], 1, 0) and s.rounds(chunk) == [(1, list(range(mp)), R.CvRng().state)]
        s, = check(programs, model, chunk, [(mp, [[]], -1)])
        assert s.result() == (-1, -1, 0, 0, MODELS[model][2], 1, 0)


@pytest.mark.parametrize("model", MODELS)
def test_fewer_points_than_the_model_needs(programs, model):
    """done from the start: never filled, alone (no round at all) or beside a live pair (idle slots only)"""
    mp, mps, max_iters, _ = MODELS[model]
    for count in (0, mp - 1):
        fills, _, results, n_rounds = _run(programs, model, 64, [(count, [[count] * mps], -1)])
        assert n_rounds == 0 and fills == [[]] and results[0] == (-1, -1, 0, 0, max_iters, 1, 0)
        check(programs, model, 64, [(count, [], -1), _planted(model, 9, {70: 100})])


@pytest.mark.parametrize("fail_at", [0, 5, 64, 70])
def test_sampler_gives_up(programs, fail_at):
    """the 4-point sampler meets a collinear set at draw j: the pair ends with iter = j and keeps the best found before j"""
    problem = (200, _planted("homography", 11, {2: 40})[1], fail_at)
    for chunk in (1, 3, 64, 1024):
        s, = check(programs, "homography", chunk, [problem])
        assert s.failed and s.iter == fail_at and s.niters == 2000 and s.best[0] == (2 if fail_at > 2 else -1)
        assert s.draws[-1][0] is None and len(s.draws) == fail_at + 1


@pytest.mark.parametrize("model", MODELS)
def test_three_pairs_finish_in_different_rounds(programs, model):
    """a batch: pair 0 ends in the first round of 64, pair 1 in the third, pair 2 in the second; finished pairs get idle slots and
    are not replayed again (their slots hold winning counts)"""
    problems = [_planted(model, 21, {10: _good_for(model, 200, 17)}, hi=4), _planted(model, 22, {40: _good_for(model, 200, 145)}, hi=4),
                _planted(model, 23, {66: _good_for(model, 150, 29)}, count=150, hi=4)]
    seqs = check(programs, model, 64, problems)
    assert [len(s.rounds(64)) for s in seqs] == [1, 3, 2] and [s.iter for s in seqs] == [17, 145, 67]
    for chunk in (3, 65):
        check(programs, model, chunk, problems)
