"""The cases of tests/merge_cases.py test something, shown without a GPU: the plain reference (tests/merge_ref.py) and the
library's two host walks agree on every one of them entry for entry, the reference's own counters say that the cases reach
what they were built to reach (walks of several hops, rejected seeds, seeds cleared by earlier images, multi-matches of four
and more key points, outcomes that depend on the seed order), and a reference with one clause of the merge turned into a
plausible mistake gives another answer on a named case.  tests/test_gpu_merge_edges.py then holds the device merge to the
same reference on the same cases."""
import numpy as np
import pytest

import merge_cases as C
from merge_ref import merge_ref
from test_merge_parallel import random_pairs, run

SMALL = [(nf, "small_model_%s_" % "".join(map(str, nf))) for nf in C.SMALL_MODELS]


def records(mm, mem):
    return [tuple(map(tuple, mem[at: at + n].tolist())) for n, at in mm.tolist()]


@pytest.mark.parametrize("name", C.CASES)
def test_reference_equals_both_host_walks(name):
    """mode 1 = upstream's literal single-threaded walk, mode 0 = the parallel one; both called directly, so the answer
    does not depend on SSRLCV_MERGE_THREADS"""
    from ssrlcv_amd import _lib
    lib = _lib.load()
    nf, blocks = C.case(name)
    mm, mem, stats = C.reference(name)
    assert len(mm) == stats["good"] and len(mem) == int(mm[:, 0].sum())
    for mode in (1, 0):
        mm_h, mem_h = run(lib, nf, blocks, mode)
        assert np.array_equal(mm_h, mm) and np.array_equal(mem_h, mem), (name, mode, len(mm_h), len(mm))


@pytest.mark.parametrize("name", C.CASES)
def test_cases_are_well_formed(name):
    """pair order, indices in range, and no query twice in a block (but for the case that is about exactly that)"""
    nf, blocks = C.case(name)
    pairs = C.pair_list(len(nf))
    assert len(blocks) == len(pairs)
    for (q, t), blk in zip(pairs, blocks):
        assert (blk["a"][:, 0] == q).all() and (blk["b"][:, 0] == t).all()
        assert (blk["a"][:, 1] < nf[q]).all() and (blk["b"][:, 1] < nf[t]).all()
        if name not in C.HOST_ONLY:
            assert len(np.unique(blk["a"][:, 1])) == len(blk)
    if name in C.HOST_ONLY:
        assert any(len(np.unique(blk["a"][:, 1])) < len(blk) for blk in blocks)


@pytest.mark.parametrize("name", list(C.HAND))
def test_hand_made_cases_give_the_arrays_written_out(name):
    _, _, mm_x, mem_x, _ = C.HAND[name]
    mm, mem, _ = C.reference(name)
    assert mm.tolist() == [list(r) for r in mm_x] and mem.tolist() == [list(r) for r in mem_x]


MIXED = [n for n in C.TRACKS if n not in ("tracks_v4_clean", "tracks_v32_full")]


@pytest.mark.parametrize("name", MIXED)
def test_mixed_tracks_reach_the_deep_walk(name):
    s = C.reference(name)[2]
    print(name, {k: v for k, v in s.items() if k != "outcome"})
    assert s["deep"] >= 100 and s["bad"] >= 100 and s["skipped_because_cleared"] >= 100 and s["ge4"] >= 100


def test_clean_tracks_are_all_accepted_in_any_order():
    s = C.reference("tracks_v4_clean")[2]
    assert s["bad"] == 0 and s["deep"] >= 300 and C.order_dependent("tracks_v4_clean") == 0


@pytest.mark.parametrize("name,depth", [("tracks_v5_mixed", 2), ("tracks_v8_mixed", 3), ("tracks_v32_mixed", 5)])
def test_hop_depth_of_the_mixed_tracks(name, depth):
    assert C.reference(name)[2]["max_depth"] >= depth


def test_full_tracks_walk_29_hops():
    """64 points in all 32 images: seed lists of 31 entries, 29 further hops down to the two-entry list of image 29"""
    nf, blocks = C.case("tracks_v32_full")
    mm, _, s = C.reference("tracks_v32_full")
    assert s["max_depth"] == 29 and s["good"] == 64 and (mm[:, 0] == 32).all()


@pytest.mark.parametrize("name", ["tracks_v6_collide", "tracks_v5_mixed"])
def test_the_seed_order_matters(name):
    assert C.order_dependent(name) >= 40


@pytest.mark.parametrize("name", ["tail_image0", "tail_image1", "tail_two_images", "tail_mixed", "chain_47", "chain_48", "chain_49"])
def test_chains_are_chains(name):
    """The reference knows nothing of rounds; what it can say is that the chain image has that many live seeds."""
    s = C.reference(name)[2]
    want = {"chain_47": 47, "chain_48": 48, "chain_49": 49}.get(name, 300)
    assert s["good"] + s["bad"] >= want
    if name == "tail_mixed":  # accepted, rejected and skipped seeds in turn, and the order decides a quarter of the chain
        assert s["good"] >= 250 and s["bad"] >= 50 and s["skipped_because_cleared"] >= 100 and C.order_dependent(name) >= 50


@pytest.mark.parametrize("nf,prefix", SMALL)
def test_small_models_hold_every_configuration(nf, prefix):
    """Every configuration "feature f of image q matches nothing or one feature of image t" in ONE problem, packed side by
    side and interleaved: the output splits into the configurations' own outputs (no multi-match crosses two of them, the
    two packings agree configuration by configuration, and every 7th configuration merged on its own gives its share).
    Distinct per-configuration outputs of the reference (MatchSet and per-seed outcome), which the bound is on:
    100, 1 419, 1 316 and 5 483 for the four models; distinct MatchSets alone: 81, 672, 891, 2 664."""
    K = C.small_model_configs(nf)
    assert K == C.SMALL_MODEL_CONFIGS[C.SMALL_MODELS.index(nf)]
    mm, mem, s = C.reference(prefix + "packed")
    mm_i, mem_i, s_i = C.reference(prefix + "interleaved")
    assert C.case(prefix + "packed")[0] == [n * K for n in nf] == C.case(prefix + "interleaved")[0]
    sets = C.per_configuration(nf, False, mm, mem)
    outcomes = C.per_configuration_outcomes(nf, False, s["outcome"])
    assert sets == C.per_configuration(nf, True, mm_i, mem_i)
    assert outcomes == C.per_configuration_outcomes(nf, True, s_i["outcome"])
    for k in range(0, K, 7):
        mm_k, mem_k, _ = merge_ref(*C.small_model_single(nf, k))
        assert tuple(records(mm_k, mem_k)) == sets[k], k
    distinct, distinct_sets = len(set(zip(sets, outcomes))), len(set(sets))
    print("%s: %d configurations, %d distinct outputs, %d distinct MatchSets" % (nf, K, distinct, distinct_sets))
    assert distinct >= (50 if nf == [2, 2, 2] else 1000)
    assert C.order_dependent(prefix + "packed") > 0


# one clause of the merge turned into a mistake -> a case whose answer it changes
MUTANT_CASES = [("never_continue", "tracks_v8_mixed"), ("follow_last", "tracks_v4_drop"), ("compare_with_prev", "tracks_v32_full"),
                ("no_clear_on_accept", "tracks_v4_clean"), ("clear_last_member_too", "tracks_v5_mixed"),
                ("never_continue", "tracks_v32_mixed"), ("follow_last", "tail_mixed"), ("no_clear_on_accept", "hand_two_ready_seeds_clear_one_list"),
                ("clear_last_member_too", "small_model_2211_interleaved"), ("compare_with_prev", "chain_49")]


@pytest.mark.parametrize("mutant,name", MUTANT_CASES)
def test_a_mutant_of_the_reference_changes_the_answer(mutant, name):
    mm, mem, _ = C.reference(name)
    mm_m, mem_m, _ = merge_ref(*C.case(name), mutant=mutant)
    assert not (np.array_equal(mm_m, mm) and np.array_equal(mem_m, mem))


def test_the_stop_at_the_last_image_matters_only_where_a_query_is_matched_twice():
    """Where no block holds a query twice a list's entries are in ascending images, one each: an entry in the last image is
    the list's last, which the clearing loop leaves out anyway -- no such input can tell the mutant from the merge (shown
    here on the deepest cases).  hand_last_image_twice can: without the stop the mutant reaches for a list of the last
    image, which owns none."""
    for name in ("tracks_v8_mixed", "tracks_v32_full", "small_model_222_packed"):
        mm, mem, _ = C.reference(name)
        mm_m, mem_m, _ = merge_ref(*C.case(name), mutant="no_stop_at_last_image")
        assert np.array_equal(mm_m, mm) and np.array_equal(mem_m, mem)
    with pytest.raises(IndexError):
        merge_ref(*C.case("hand_last_image_twice"), mutant="no_stop_at_last_image")


def test_the_reversed_seed_order_changes_the_answer():
    """as sets of multi-matches: the reversed walk also emits in reversed order, which alone would differ"""
    name = "tracks_v6_collide"
    mm, mem, _ = C.reference(name)
    mm_r, mem_r, _ = merge_ref(*C.case(name), reverse=True)
    assert set(records(mm_r, mem_r)) != set(records(mm, mem))
    mm_c, mem_c, _ = C.reference("tracks_v4_clean")
    mm_r, mem_r, _ = merge_ref(*C.case("tracks_v4_clean"), reverse=True)
    assert set(records(mm_r, mem_r)) == set(records(mm_c, mem_c))  # ... and only there


def test_what_random_pairs_reaches():
    """Why the cases above exist: the generator of test_merge_parallel.py / test_gpu_merge.py hardly ever makes a walk
    take a second hop.  Printed, not asserted (run with -s)."""
    for V, n, density, spread in [(4, 3000, 0.6, 3000), (4, 5000, 0.7, 40), (6, 800, 0.8, 25), (8, 400, 0.5, 400), (12, 300, 0.7, 60),
                                  (32, 120, 0.4, 50)]:
        rng = np.random.default_rng(V * 1000 + n)
        nf = [int(n * (0.7 + 0.6 * rng.random())) for _ in range(V)]
        s = merge_ref(nf, random_pairs(rng, nf, density, min(spread, min(nf))))[2]
        print("random_pairs V=%d n=%d spread=%d: %d seeds walked, %d deep, max depth %d, %d of 4+ key points" %
              (V, n, spread, s["good"] + s["bad"], s["deep"], s["max_depth"], s["ge4"]))
    for name in C.TRACKS:
        s = C.reference(name)[2]
        print("%s: %d seeds walked, %d deep, max depth %d, %d of 4+ key points" % (name, s["good"] + s["bad"], s["deep"], s["max_depth"], s["ge4"]))
