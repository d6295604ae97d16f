"""Image retrieval on the GPU (esfm.h "Image retrieval") against the numpy restatement (tests/retrieval_ref.py), bit for bit, stage
by stage: centres, assign, sums, vlad, norm2, dots, scores (as bit patterns), nearest and the pair list -- at the matrix
instruction's tile edges, on both sides of the LDS / global accumulation switch, with duplicate centres and empty clusters, and
on the degenerate images the rule list names."""
import functools

import numpy as np
import pytest

import retrieval_cases as cases
import retrieval_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import easysfm_amd
    return easysfm_amd


def hamming_sets(n_sets, nbytes, seed):
    from easysfm_amd import synth
    sets = synth.orb_like_sets(n_sets, 70, pool=256, seed_base=seed, nbytes=nbytes)
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(s[:int(rng.integers(40, 71))]) for s in sets]


# name: (metric, sets, options).  D = n_centres * d; the sums are gathered in LDS up to D = 6144 and by global atomics above.
@functools.lru_cache(maxsize=None)
def case(name):
    o = R.Options
    table = {
        "one_set_width1": lambda: (R.L2, cases.float_sets(1, 1, 1), o(n_centres=1, top_k=2)),
        "two_sets_width3": lambda: (R.L2, cases.float_sets(2, 3, 2), o(n_centres=2, top_k=1)),
        "n15_w64_c64_lds": lambda: (R.L2, cases.float_sets(15, 64, 3), o(n_centres=64, top_k=4)),                 # D = 4096: LDS
        "n16_w65_c3": lambda: (R.L2, cases.float_sets(16, 65, 4), o(n_centres=3, top_k=3)),                      # D = 195
        "n17_w128_c64_global": lambda: (R.L2, cases.float_sets(17, 128, 5), o(n_centres=64, top_k=5)),            # D = 8192: global atomics
        "n33_w5_c3_edges": lambda: (R.L2, cases.float_sets(33, 5, 6, empty=7, single=20, long=11), o(n_centres=3, top_k=6, window=1)),   # D = 15
        "n16_w4_c16_D64": lambda: (R.L2, cases.float_sets(16, 4, 7), o(n_centres=16, top_k=3)),                   # D = 64 exactly
        "hamming16_c16_lds": lambda: (R.HAMMING, hamming_sets(17, 16, 3100), o(n_centres=16, top_k=4)),           # d = 128, D = 2048
        "hamming32_c64_global": lambda: (R.HAMMING, hamming_sets(15, 32, 3200), o(n_centres=64, top_k=4)),        # d = 256, D = 16384
        "centres_beyond_sample": lambda: (R.L2, cases.float_sets(2, 3, 8, rows=(40, 40)), o(n_centres=16, max_train=5, top_k=1)),   # nt = 5 < 16
        "stride_above_one": lambda: (R.L2, cases.float_sets(15, 64, 9), o(n_centres=16, max_train=100, top_k=4)),
        "no_iterations": lambda: (R.L2, cases.float_sets(5, 8, 10), o(n_centres=8, kmeans_iterations=0, top_k=2)),
        "identical_images_and_rows": lambda: (R.L2, cases.identical_rows_case(), o(n_centres=8, top_k=4)),
        "top_k_beyond_n": lambda: (R.L2, cases.float_sets(5, 8, 11), o(n_centres=4, top_k=10)),
        "window_alone": lambda: (R.L2, cases.float_sets(6, 8, 12), o(n_centres=4, top_k=0, window=2)),
    }
    metric, sets, opt = table[name]()
    return metric, sets, opt, R.chain(sets, metric, opt)


NAMES = ["one_set_width1", "two_sets_width3", "n15_w64_c64_lds", "n16_w65_c3", "n17_w128_c64_global", "n33_w5_c3_edges", "n16_w4_c16_D64",
         "hamming16_c16_lds", "hamming32_c64_global", "centres_beyond_sample", "stride_above_one", "no_iterations", "identical_images_and_rows",
         "top_k_beyond_n", "window_alone"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("name", NAMES)
def test_stages_match_the_restatement(E, gpu_ctx, name):
    metric, sets, o, ref = case(name)
    opt = E.RetrievalOptions(**o.kw)
    centres = E.retrieval_train(sets, metric, opt, gpu_ctx)
    assert same_bits(centres, ref["centres"]), "centres"
    # the later stages take the restatement's codebook, so that each is pinned on its own
    vlad, norm2, assign, sums = E.retrieval_vlad(sets, ref["centres"], metric, gpu_ctx, debug=True)
    assert np.array_equal(assign, ref["assign"]), "assign"
    assert np.array_equal(sums, ref["sums"]), "sums"
    assert same_bits(vlad, ref["vlad"]) and np.array_equal(norm2, ref["norm2"]), "vlad / norm2"
    nearest, dots, scores = E.retrieval_rank(ref["vlad"], o.top_k, gpu_ctx, debug=True)
    assert np.array_equal(dots, ref["dots"]), "dots"
    assert same_bits(scores, ref["scores"]), "scores"
    assert np.array_equal(nearest, ref["nearest"]), "nearest"
    assert np.array_equal(E.retrieval_pair_list(nearest if o.top_k else None, len(sets), o.window), ref["pairs"])
    assert np.array_equal(E.select_pairs(sets, metric, opt, gpu_ctx), ref["pairs"]), "the whole chain"


def test_cases_are_what_they_claim():
    """the restatement's answers have the properties the cases were built for"""
    _, sets, o, ref = case("centres_beyond_sample")
    m = ref["centres"]
    assert len({m[c].tobytes() for c in range(16)}) <= 5 and len(np.unique(ref["assign"])) <= 5      # duplicates; empty clusters keep their value
    _, sets, o, ref = case("identical_images_and_rows")
    assert ref["norm2"][3] == 0 and np.all(ref["nearest"][3] == -1) and not np.any(ref["nearest"] == 3)
    assert np.array_equal(ref["vlad"][2], ref["vlad"][4]) and ref["scores"][0, 2] == ref["scores"][0, 4]
    row0 = list(ref["nearest"][0])
    assert 2 in row0 and 4 in row0 and row0.index(2) + 1 == row0.index(4)                            # equal scores: index order
    _, sets, o, ref = case("top_k_beyond_n")
    assert len(ref["pairs"]) == 10 and np.all(ref["nearest"][:, 4:] == -1) and np.all(ref["nearest"][:, :4] >= 0)   # every pair of five images
    _, sets, o, ref = case("window_alone")
    assert [tuple(p) for p in ref["pairs"]] == [(i, i - w) for i in range(6) for w in (2, 1) if i - w >= 0]
    _, sets, o, ref = case("n33_w5_c3_edges")
    assert len(sets[7]) == 0 and len(sets[20]) == 1 and len(sets[11]) == 1100
    assert ref["norm2"][7] == 0 and np.all(ref["nearest"][7] == -1)                                  # an image without rows
    _, sets, o, ref = case("stride_above_one")
    assert len(R.sample_rows(sum(len(s) for s in sets), o.max_train)) < sum(len(s) for s in sets)


def test_one_hot_descriptors_pin_the_operand_layout(E, gpu_ctx):
    """int8 rows with one or two non-zero entries, given straight to esfm_retrieval_rank: every dot product is one or two products
    of entries at the same k, so an operand whose k order differed between the two sides, or a result read from the wrong lane,
    shows in the table; n = 33 and D = 200 leave a ragged tile on both axes"""
    V = cases.one_hot_vlads()
    ref_nearest, ref_dots, ref_scores = R.rank(V, 5)
    assert np.count_nonzero(ref_dots - np.diag(np.diagonal(ref_dots))) > 20
    nearest, dots, scores = E.retrieval_rank(V, 5, gpu_ctx, debug=True)
    assert np.array_equal(dots, ref_dots)
    assert same_bits(scores, ref_scores) and np.array_equal(nearest, ref_nearest)
    # a descriptor with every entry set, against unit vectors: row i of the table is V's column pattern itself
    W = np.zeros((17, 128), np.int8)
    W[0] = (np.arange(128) % 100) - 50
    W[1:, :] = 0
    for i in range(1, 17):
        W[i, 8 * (i - 1) + (i % 8)] = 1
    _, dots, _ = E.retrieval_rank(W, 1, gpu_ctx, debug=True)
    assert np.array_equal(dots, R.rank(W, 1)[1])


def test_row_order_inside_an_image_does_not_matter(E, gpu_ctx):
    """with the codebook supplied, shuffling the rows inside every image leaves vlad and norm2 unchanged: integer sums"""
    metric, sets, o, ref = case("n17_w128_c64_global")
    rng = np.random.default_rng(1)
    shuffled = [s[rng.permutation(len(s))] for s in sets]
    vlad, norm2 = E.retrieval_vlad(shuffled, ref["centres"], metric, gpu_ctx)
    assert same_bits(vlad, ref["vlad"]) and np.array_equal(norm2, ref["norm2"])
    metric, sets, o, ref = case("n33_w5_c3_edges")
    shuffled = [s[rng.permutation(len(s))] for s in sets]
    vlad, norm2 = E.retrieval_vlad(shuffled, ref["centres"], metric, gpu_ctx)
    assert same_bits(vlad, ref["vlad"]) and np.array_equal(norm2, ref["norm2"])


def test_corridor_three_ways(E, gpu_ctx):
    """esfm_retrieval_pairs, esfm_retrieval_pairs_dev over a DescriptorBank and the chain of stage calls give the same list on the
    corridor scene, the restatement's; so the GPU's table meets the conditions tests/test_retrieval_cpu.py puts on retrieval"""
    sets, ids = cases.corridor(11)
    o = R.Options(n_centres=16, kmeans_iterations=10, top_k=4, window=1)
    opt = E.RetrievalOptions(**o.kw)
    ref = R.chain(sets, R.L2, o)
    host = E.select_pairs(sets, R.L2, opt, gpu_ctx)
    bank = E.DescriptorBank(sets, R.L2)
    resident = E.select_pairs(bank, R.L2, opt, gpu_ctx)
    centres = E.retrieval_train(sets, R.L2, opt, gpu_ctx)
    vlad, norm2 = E.retrieval_vlad(sets, centres, R.L2, gpu_ctx)
    nearest, dots, scores = E.retrieval_rank(vlad, o.top_k, gpu_ctx, debug=True)
    staged = E.retrieval_pair_list(nearest, len(sets), o.window)
    assert np.array_equal(host, ref["pairs"]) and np.array_equal(resident, ref["pairs"]) and np.array_equal(staged, ref["pairs"])
    assert np.array_equal(nearest, ref["nearest"]) and same_bits(scores, ref["scores"])
    cases.check_corridor(nearest, scores, ids)


def test_stage_times_are_reported(E, gpu_ctx):
    """under the context's kernel timing the last chain call reports a device time for each of its four stages"""
    from easysfm_amd import retrieval
    metric, sets, o, ref = case("n15_w64_c64_lds")
    gpu_ctx.set_kernel_timing(True)
    try:
        pairs = E.select_pairs(sets, metric, E.RetrievalOptions(**o.kw), gpu_ctx)
        ms = retrieval.last_stage_ms(gpu_ctx)
    finally:
        gpu_ctx.set_kernel_timing(False)
    assert np.array_equal(pairs, ref["pairs"])
    assert len(ms) == 4 and all(0.0 < v < 1000.0 for v in ms), ms
    assert E.lib().esfm_retrieval_last_stage_ms(gpu_ctx.handle, None) == -1


def test_resident_rows_are_validated(E, gpu_ctx):
    """esfm_retrieval_pairs_dev cannot look at the rows on the host: a value beyond the fixed point's range is found on the device"""
    sets = cases.float_sets(3, 4, 13)
    sets[1][5, 2] = np.inf
    bank = E.DescriptorBank(sets, R.L2)
    with pytest.raises(E.EsfmError) as ei:
        E.select_pairs(bank, R.L2, E.RetrievalOptions(n_centres=2, top_k=1), gpu_ctx)
    assert ei.value.status == -1 and "16384" in str(ei.value)
