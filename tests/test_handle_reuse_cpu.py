"""CPU rehearsal of tests/test_gpu_handle_reuse.py: bookkeeping on the schedules and inputs of tests/handle_reuse_cases.py.  A schedule
that silently lost its point -- a pair of drivers never adjacent, a batch that no longer flips the hit-mask path, a type that exists in
one size only -- fails here, without a GPU."""
import numpy as np
import pytest

import handle_reuse_cases as hc


def _sizes(kind, sched, golden):
    return [hc.totals(hc.inputs(kind, t, s, golden)) for t, s in sched]


@pytest.mark.parametrize("kind", hc.FULL_KINDS)
def test_full_schedule_has_every_ordered_pair_and_every_neighbor_relation(kind):
    sched = hc.full_schedule(kind)
    types = [t for t, _ in sched]
    pairs = set(zip(types[:-1], types[1:]))
    assert len(hc.SHARED) == 8 and len(hc.euler_walk(list(hc.SHARED))) == 65
    missing = [(a, b) for a in hc.SHARED for b in hc.SHARED if (a, b) not in pairs]
    assert not missing, missing
    for z in hc.SPECIAL + ("Mr",):
        for near in ("F", "E"):
            assert (near, z) in pairs and (z, near) in pairs, (z, near)
    assert len(sched) >= 65 + 5 * len(hc.SPECIAL)
    assert set(types) == set(hc.TYPES)
    # W twice, each directly followed by an S-sized episode
    w = [i for i, (_, s) in enumerate(sched) if s == "W"]
    assert len(w) == 2 and all(sched[i][0] == "E" and sched[i + 1][1] == "S" for i in w)
    # K before most of the schedule: what follows runs on the tight pool
    assert types.index("K") < len(types) // 2


@pytest.mark.parametrize("kind", hc.FULL_KINDS)
def test_full_schedule_alternates_sizes_and_reaches_every_type_from_both_sides(kind, golden):
    sched = hc.full_schedule(kind)
    cls = [hc.size_class(s) for _, s in sched]
    assert all(a != b for a, b in zip(cls[:-1], cls[1:]))
    tot = _sizes(kind, sched, golden)
    for t in hc.TYPES:
        at = [i for i, (x, _) in enumerate(sched) if x == t and i > 0]
        assert {s for x, s in sched if x == t} >= {"S", "G"}, t
        assert any(tot[i - 1][0] > tot[i][0] and tot[i - 1][1] > tot[i][1] for i in at), (t, "never after a larger batch")
        assert any(tot[i - 1][0] < tot[i][0] and tot[i - 1][1] < tot[i][1] for i in at), (t, "never after a smaller batch")


@pytest.mark.parametrize("kind", hc.REDUCED_KINDS + hc.PAINN_KINDS)
def test_reduced_schedule_has_every_applicable_type_in_both_sizes(kind):
    sched = hc.reduced_schedule(kind)
    assert sched == hc.reduced_schedule(kind)                      # a seeded shuffle: the same order every time
    body = sched[:2 * len(hc.APPLICABLE[kind])]
    assert sorted(body) == sorted((t, s) for t in hc.APPLICABLE[kind] for s in ("S", "G"))
    assert all(hc.size_class(a[1]) != hc.size_class(b[1]) for a, b in zip(body[:-1], body[1:]))
    assert any(t == "K" for t, _ in body[:len(body) // 2])
    assert set(hc.APPLICABLE[kind]) <= set(hc.TYPES)
    if kind == "painn":
        tail = sched[len(body):]
        assert tail == list(hc.PAINN_TAIL)
        after = {tail[i][1]: tail[i + 1][1] for i in range(len(tail) - 1) if tail[i][1] != "S"}
        assert tail[0][1] == "big960" and tail[1][1] == "S"
        assert ("sp2", "S") in zip([s for _, s in tail], [s for _, s in tail][1:])          # 2 species, then the 3-species slab again
        assert ("sp9", "sp2") in zip([s for _, s in tail], [s for _, s in tail][1:])
        assert ("S", "sp9") in zip([s for _, s in tail], [s for _, s in tail][1:])
        assert after["sp1"] == "S"
    else:
        assert len(sched) == len(body)


@pytest.mark.parametrize("kind", hc.KINDS)
def test_image_grids_switch_the_hit_masks_on_and_off(kind, golden):
    rc = hc.cutoff(kind)
    S, G = hc.inputs(kind, "E", "S", golden), hc.inputs(kind, "E", "G", golden)
    gs, gg = [hc.image_grid(s, rc) for s in S.structs], [hc.image_grid(s, rc) for s in G.structs]
    assert max(gs) <= 64, gs
    assert max(gg) > 64 and min(gg) <= 64, gg
    assert len(S.structs) == 2 and len(G.structs) == 5
    if kind not in hc.PAINN_KINDS + ("ewald",):
        assert [len(s[0]) for s in S.structs] == [8, 8] and tuple(len(s[0]) for s in G.structs) == hc.G_SIZES
        assert any(not np.asarray(s[3]).all() for s in G.structs)              # open axes next to periodic ones
    for t in ("P", "X"):
        if t in hc.APPLICABLE[kind]:
            Gp = hc.inputs(kind, t, "G", golden)
            assert all(np.asarray(s[3]).all() for s in Gp.structs)             # a barostat / a strain wants periodic cells
            assert max(hc.image_grid(s, rc) for s in Gp.structs) > 64
            assert max(hc.image_grid(s, rc) for s in hc.inputs(kind, t, "S", golden).structs) <= 64


def _all_inputs(kind, golden):
    seen = {}
    for t, s in hc.schedule(kind):
        seen[(t if t in hc.STRUCTURED + ("P", "X") else "generic", s)] = hc.inputs(kind, t, s, golden)
    return seen


@pytest.mark.parametrize("kind", hc.KINDS)
def test_chain_sizes(kind, golden):
    for (t, s), inp in _all_inputs(kind, golden).items():
        n = [len(x[0]) for x in inp.structs]
        assert len(inp.held) == len(inp.mass) == sum(n)
        if s == "big960":
            assert n == [960] and hc.BIG_CHAIN_RANGE[0] <= n[0] <= hc.BIG_CHAIN_RANGE[1]
        else:
            assert max(n) <= 256, (t, s, n)
        if s == "W":
            assert sum(n) > 4096
    if kind in hc.FULL_KINDS:
        assert ("generic", "W") in _all_inputs(kind, golden)


def test_painn_species_batches(golden):
    count = lambda name: len(set(np.concatenate([s[0] for s in hc.painn_extra(name, golden)]).tolist()))     # noqa: E731
    assert [count(n) for n in ("sp1", "sp2", "sp9")] == [1, 2, 9]
    assert len(set(np.concatenate([s[0] for s in hc.inputs("painn", "E", "S", golden).structs]).tolist())) == 3


@pytest.mark.parametrize("kind", hc.KINDS)
def test_structured_inputs_come_in_a_smaller_and_a_larger_size(kind, golden):
    S = hc.totals(hc.inputs(kind, "E", "S", golden))
    for t in hc.STRUCTURED:
        if t not in hc.APPLICABLE[kind]:
            continue
        small, large = hc.inputs(kind, t, "S", golden), hc.inputs(kind, t, "G", golden)
        assert hc.totals(small)[0] < S[0], (t, hc.totals(small), S)
        assert hc.totals(large)[0] > S[0] and hc.totals(large)[1] > S[1], (t, hc.totals(large), S)
        if t == "V":
            assert max(small.extra["n_rep"]) > 1 and max(large.extra["n_rep"]) > 1
            assert sum(small.extra["n_rep"]) == len(small.structs) and sum(large.extra["n_rep"]) == len(large.structs)
        if t == "N":
            assert small.extra["n_img"] == [len(small.structs)] and min(large.extra["n_img"]) >= 3
        if t == "D":
            assert len(small.structs) % 2 == 0 and len(large.structs) % 2 == 0


@pytest.mark.parametrize("kind", hc.KINDS)
def test_no_pair_sits_on_a_cutoff(kind, golden):
    """No pair of any input within 1e-6 relative of a distance at which a term switches: bit equality cannot hinge on a boundary."""
    assert min(hc.term_cutoffs(kind)) > 0
    worst = min(hc.cutoff_margin(kind, s) for inp in _all_inputs(kind, golden).values() for s in inp.structs)
    assert worst > 1e-6, worst


def test_every_parameter_set_is_one_the_front_end_accepts():
    from surface_sampling_amd import backend

    p = hc.c_params(backend)
    assert p["fire"].max_steps == hc.FIRE["max_steps"] and p["bfgs"].max_steps == hc.BFGS["max_steps"]
    assert p["cg"].max_iter == hc.CG["max_iter"] and p["bfgsls"].max_eval == 20 * hc.BFGSLS["max_steps"] + 20
    assert p["npt"].barostat == backend.NPT_BAROSTATS["berendsen"] and p["npt"].n_steps == hc.NPT["steps"]
    assert p["cell"].max_steps == hc.CELL["max_steps"] and p["neb"].climb == 1 and p["dimer"].seed == hc.DIMER["seed"]
    assert p["vib"].nfree == 2 and p["md"].thermostat == backend.MD_THERMOSTATS["langevin"]
    assert backend.cg_driver_code("lockstep") == 1 and backend.md_driver_code("resident") == 2
    # the refused arguments of R are refused by the library, not by the front end: the front end passes them on
    assert backend.VibParams(3, 0, 0.01, 0.0, 0.0).nfree == 3


def test_first_difference_names_the_output_and_the_chain():
    inp = hc.Inputs([(np.zeros(2, np.int32),) * 1, (np.zeros(3, np.int32),) * 1], None, None, {})
    a = [("e", np.zeros(2)), ("f", np.zeros((5, 3))), ("traj", np.zeros((4, 5, 3)))]
    assert hc.first_difference(a, [(n, x.copy()) for n, x in a], inp) is None
    b = [(n, x.copy()) for n, x in a]
    b[1][1][3, 0] = np.nan
    assert hc.first_difference(a, b, inp) == ("f", "bytes differ", 1)
    assert hc.first_difference(b, [(n, x.copy()) for n, x in b], inp) is None          # NaNs compare equal as bytes
    c = [(n, x.copy()) for n, x in a]
    c[2][1][1, 1, 2] = 1.0
    assert hc.first_difference(a, c, inp) == ("traj", "bytes differ", 0)
    assert hc.first_difference(a, a[:2], inp)[0] == "(the list of outputs)"
    assert hc.first_difference(a, [("e", np.zeros(2, np.float32))] + a[1:], inp)[0] == "e"
