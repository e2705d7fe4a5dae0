"""Bit-equality record of the PaiNN 128 / 20 pipeline: evaluates a fixed set of small cases on the library VSSR_EVAL_LIB names (as
every tool here) and prints one JSON object {case: {array: SHA-256 of its bytes}}.  Run it once per build and diff the outputs: a
refactor of painn.hip / painn_edge_mfma.hip / painn_l0.hip / painn_node_mfma.hip / api_batch.hip must leave every digest as it was.

Digested per case: energy, energy_f64, energy_std, energy_models, forces, forces_std, the per-atom energies and the stress (mean
and spread over the models).

Cases (the smallest that reach every host branch and reverse-pass kernel of those files):
  ragged_*        the four 76 .. 270-atom structures of test_narrow_feature_slices_match_the_oracle_on_the_small_structures as one
                  batch: default settings; that test's six knob sets (8- and 4-feature slices, both forward multi-pass forms, the
                  reverse multi-pass form with ranges of 100 and 70 atoms, 4- and 8-wave launches); VSSR_EDGE_FS16_MAX=100 (two slice
                  classes in one batch: the per-chain form of the partial-gradient reduction); VSSR_L0_FACTORISE=0 (layer 0 on the
                  gather kernels, next to matrix-pipe layers); VSSR_EDGE_IMPL=gather (no partial buffers at all);
                  VSSR_PAINN_PATH=general (the general-width path's use of the shared finalize code)
  single_chain / single_class   one chain; two chains of one class (the uniform form of the reduction)
  energy_only     no reverse pass
  fire_masked     6 lock-step FIRE steps of two chains, one of them held fixed entirely: the driver learns at its first poll (after
                  four evaluations) that this chain has stopped and hands the active mask to the last three evaluations; "masked" (in
                  clear) is true when that happened -- the batch is then left with a partial graph and stress() refuses
  gather_next_to_mfma   a 1 500-atom chain (gather class: beyond the 1 462 atoms of the matrix-pipe classes) next to a 76-atom one
  num_conv_1 / num_conv_2   the shipped weights cut to one and two message / update blocks (tests/painn_shapes.py)
Usage: VSSR_EVAL_LIB=build/variants/lib_x.so python tools/dump_painn.py > out.json"""
import hashlib, json, os, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = {}
KEYS = ("energy", "energy_f64", "energy_std", "energy_models", "forces", "forces_std", "energy_atoms")

KNOB_SETS = {
    "default": {},
    "fs8": {"VSSR_EDGE_FS16_MAX": "0"},
    "fs4_fwd16": {"VSSR_EDGE_FS16_MAX": "0", "VSSR_EDGE_FS8_MAX": "0"},
    "fs4_fwd8": {"VSSR_EDGE_FS16_MAX": "0", "VSSR_EDGE_FS8_MAX": "0", "VSSR_EDGE_FWD_2PASS": "8"},
    "fs4_both": {"VSSR_EDGE_FS16_MAX": "0", "VSSR_EDGE_FS8_MAX": "0", "VSSR_EDGE_FWD_2PASS": "0"},
    "mpass_100": {"VSSR_EDGE_FS16_MAX": "0", "VSSR_EDGE_FS8_MAX": "0", "VSSR_EDGE_BWD_MPASS": "2", "VSSR_EDGE_SUB_CHUNK": "100"},
    "mpass_70_fwd8": {"VSSR_EDGE_FS16_MAX": "0", "VSSR_EDGE_FS8_MAX": "0", "VSSR_EDGE_BWD_MPASS": "2", "VSSR_EDGE_SUB_CHUNK": "70",
                      "VSSR_EDGE_FWD_2PASS": "8"},
    "two_classes": {"VSSR_EDGE_FS16_MAX": "100"},
    "l0_gather": {"VSSR_L0_FACTORISE": "0"},
    "gather": {"VSSR_EDGE_IMPL": "gather"},
    "general": {"VSSR_PAINN_PATH": "general"},
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(case, res, **more):
    OUT[case] = {k: sha(res[k]) for k in KEYS if k in res}
    OUT[case].update({k: sha(v) for k, v in more.items()})


def engine(blobs, knobs=None, **kw):
    """A PaiNN engine created under ``knobs`` (the library reads them at create only)."""
    from surface_sampling_amd import backend

    knobs = knobs or {}
    os.environ.update(knobs)
    try:
        return backend.PainnEngine(blobs, device=0, **kw)
    finally:
        for k in knobs:
            del os.environ[k]


def single_point(case, eng, structs):
    res = eng.evaluate(structs)
    st, sd = eng.stress()
    record(case, res, stress=st, stress_std=sd)


def main():
    import painn_shapes
    from surface_sampling_amd import backend, structures
    from surface_sampling_amd.calculators import stoich_offset_table

    blobs = [np.fromfile(os.path.join(GOLDEN, "weights", f"SrTiO3_painn_model0{m}.f32"), dtype="<f4") for m in (1, 2, 3)]
    with open(os.path.join(GOLDEN, "offset_data.json")) as fh:
        table, const = stoich_offset_table(json.load(fh))
    S = np.load(os.path.join(GOLDEN, "structures.npz"))

    def golden(name):
        return structures.Structure(S[f"{name}.numbers"], S[f"{name}.positions"], S[f"{name}.cell"], S[f"{name}.pbc"])

    def arrays(s):
        return (s.numbers, s.positions, s.cell, s.pbc)

    base = golden("SrTiO3_2x2_pristine")
    big = base.repeat((2, 2, 1))
    ragged = [arrays(c) for c in (golden("O44Sr12Ti16"), structures.synth_chain(big, 3), structures.synth_chain(big, 17),
                                  structures.synth_chain(base, 2, grid=(4, 4)))]
    off = dict(offset_per_z=table, offset_const=const)

    for name, knobs in KNOB_SETS.items():
        eng = engine(blobs, knobs, **off)
        single_point("ragged_" + name, eng, ragged)
        eng.close()

    eng = engine(blobs, **off)
    single_point("single_chain", eng, ragged[:1])
    single_point("single_class", eng, ragged[1:3])
    res = eng.evaluate(ragged, want=backend.WANT_ENERGY | backend.WANT_STD | backend.WANT_PER_MODEL | backend.WANT_PER_ATOM)
    record("energy_only", {k: v for k, v in res.items() if not k.startswith("forces")})

    two = [ragged[3], ragged[0]]
    fixed = np.concatenate([np.ones(len(two[0][0]), np.uint8), np.arange(len(two[1][0])) % 4 == 0]).astype(np.uint8)
    eng.upload(two)
    out = eng.relax("FIRE", fixed=fixed, max_steps=6, fmax=0.01)
    record("fire_masked", eng.download(), positions=out["positions"], n_steps=out["n_steps"], converged=out["converged"])
    try:
        eng.stress()
        OUT["fire_masked"]["masked"] = False
    except backend.BackendError:
        OUT["fire_masked"]["masked"] = True

    huge = base.repeat((5, 5, 1))   # 1 500 atoms
    huge.positions += np.random.default_rng(3).normal(0, 0.03, huge.positions.shape)
    single_point("gather_next_to_mfma", eng, [arrays(huge), ragged[0]])
    eng.close()

    for L in (1, 2):
        cut, hp = painn_shapes.reshape_ensemble(blobs, 128, 20, num_conv=L)
        eng = engine(cut, hparams={"num_conv": hp["num_conv"]}, **off)
        single_point(f"num_conv_{L}", eng, ragged)
        eng.close()
    print(json.dumps(OUT, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
