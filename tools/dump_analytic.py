"""Bit-equality record of the fp64 analytic potentials and the relaxation drivers: evaluates a fixed set of small cases on the library VSSR_EVAL_LIB names (as
every tool here) and prints one JSON object {case: {array: SHA-256 of its bytes}}.  Run it once per build and diff the outputs: a
refactor of tersoff.hip / sw.hip / pair.hip / eam.hip / pot_common.hip / relax.hip / relax_cg.hip / chain_min.hip or of a driver
(relax_bfgsls.hip, md.hip, vib.hip, neb.hip, dimer.hip, relax_cell.hip) must leave every digest as it was.

Cases (the smallest that reach every kernel and branch of those files):
  tersoff_gan       GaN.tersoff: the 3x3 slab + 12 Ga adatoms (48 atoms), the bare slab (36), a 43-atom dense box whose rows
                    exceed the 16-slot tile -- three chains of unequal length, 127 atoms (no multiple of 64)
  tersoff_5species  synthetic five-species entries: more than the LDS kernel holds, every row takes the one-thread form
  sw_si111 / sw_3species   the Si(111) 5x5 slab (100 atoms); one dense three-species cell (long-row form)
  eam_funcfl / eam_alloy / eam_fs   Cu(100) and Au(110) with adatoms: Cu_u3 funcfl handle, a Cu/Au eam/alloy and an eam/fs handle
  pair_rocksalt     the 64-atom rocksalt cell with Born + coul/dsf
each with energies, per-atom energies, forces and stress(); relax_*: chain-resident CG, lock-step CG (VSSR_CG_FUSED=0), FIRE and BFGS
of the GaN batch with positions, energies and step counts; *_tight: the Tersoff and pair cases and relaxations again after
debug_capacity(tight=1) with one slot per atom, so the first run overflows and the capacity is regrown (vssr_synchronize, the
lock-step relaxation drivers).  Beyond those, on the GaN batch (whose chains stop at different polls):
  relax_cg_compact  lock-step CG with the live-chain compaction forced (VSSR_RELAX_COMPACT=2, VSSR_CG_FUSED=0), with relax_counts in clear:
                    fewer dispatched chain-evaluations than lock-step evaluations x chains = a compaction happened
  traj_fire / traj_bfgs   FIRE and BFGS with record_interval=3: the trajectory records (n_records, positions, forces, energies)
and one PaiNN (fp32) handle, the drivers' other force path:
  painn_fire / painn_bfgs   two 60-atom SrTiO3 chains with different FixAtoms masks, 6 steps
and the other drivers, each at the smallest shape that reaches its host branches, on the GaN handle (gan_*, and gan_*_tight where the
capacity is regrown inside the driver's loop or the chain-resident pools double) and on the PaiNN handle (painn_*), every returned
array plus relax_counts(), and the regrow count in clear:
  bfgsls            BFGSLineSearch, 6 steps
  md_{lockstep,resident}_{nve,langevin}   6 steps from drawn velocities, a thermo record every 2 (resident: the GaN handle only)
  vib               three chains, n_rep = [2, 1]: a replica group and a single chain, 4 vib atoms each
  neb               a band of 3 images and a band of 4 in one batch, 5 steps
  dimer             two dimers, drawn modes, 4 steps
  cell_hydrostatic / cell_slab   relax_cell of a fully periodic chain with hydrostatic strain; of two chains under the slab mask
Usage: VSSR_EVAL_LIB=build/variants/lib_x.so python tools/dump_analytic.py > out.json"""
import hashlib, json, os, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = {}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(case, **arrays):
    OUT[case] = {k: sha(v) for k, v in arrays.items()}


def single_point(case, eng, structs, tight=False):
    if tight:
        eng.debug_capacity(slots_per_atom=1, tight=1)
    e, ea, f = eng.evaluate_f64(structs)
    record(case, energy=e, e_atom=ea, forces=f, stress=eng.stress()[0])


def with_adatoms(name, every):
    """(positions, cell, pbc) of a golden slab with an adatom on every ``every``-th adsorption site."""
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return np.concatenate([d["positions"], d["ads_coords"][::every]]), d["cell"], d["pbc"].astype(np.uint8)


def gan_batch():
    import sw_oracle as so

    S = np.load(os.path.join(GOLDEN, "structures.npz"))
    Z, X, Cl = S["GaN_3x3_pristine.numbers"], S["GaN_3x3_pristine.positions"], S["GaN_3x3_pristine.cell"]
    pbc = S["GaN_3x3_pristine.pbc"].astype(np.uint8)
    T = np.where(Z == 31, 0, 1).astype(np.int32)
    ztop = X[:, 2].max()
    ads = np.array([(i + 0.5) / 4 * Cl[0] + (j + 0.5) / 3 * Cl[1] for i in range(4) for j in range(3)])
    ads[:, 2] = ztop + 1.8
    rng = np.random.default_rng(12)
    slab48 = (np.concatenate([T, np.zeros(12, np.int32)]), np.concatenate([X, ads]) + rng.normal(0, 0.05, (48, 3)), Cl, pbc)
    return [slab48, (T, X + rng.normal(0, 0.05, X.shape), Cl, pbc), so.dense_box(n=43, box=6.5, min_dist=1.55, seed=3, nt=2)]


def relaxations(eng, structs, tag, tight):
    def fresh():
        if tight:
            eng.debug_capacity(slots_per_atom=1, tight=1)

    fixed = np.concatenate([np.arange(len(s[0])) % 5 == 0 for s in structs]).astype(np.uint8)
    for name, fused in (("cg_chain", "1"), ("cg_lockstep", "0")):
        os.environ["VSSR_CG_FUSED"] = fused   # (read by the library at every call)
        fresh()
        e, ea, f, pos, it, ev, why = eng.relax_cg_f64(structs, fixed=fixed, max_iter=40, etol=0.0, ftol=1e-4)
        record(f"relax_{name}{tag}", energy=e, e_atom=ea, forces=f, positions=pos, n_iter=it, n_eval=ev, stop=why,
               regrows=np.int32(eng.debug_capacity()))
    del os.environ["VSSR_CG_FUSED"]
    for opt in ("FIRE", "BFGS"):
        fresh()
        e, ea, f, pos, steps, conv = eng.relax_f64(structs, fixed=fixed, max_steps=30, fmax=0.01, optimizer=opt)
        record(f"relax_{opt.lower()}{tag}", energy=e, e_atom=ea, forces=f, positions=pos, n_steps=steps, converged=conv,
               regrows=np.int32(eng.debug_capacity()))


def relaxations_beyond(eng, structs):
    """Forced compaction in the CG driver; trajectory records of FIRE / BFGS."""
    fixed = np.concatenate([np.arange(len(s[0])) % 5 == 0 for s in structs]).astype(np.uint8)
    os.environ.update(VSSR_CG_FUSED="0", VSSR_RELAX_COMPACT="2")
    e, ea, f, pos, it, ev, why = eng.relax_cg_f64(structs, fixed=fixed, max_iter=40, etol=0.0, ftol=1e-4)
    record("relax_cg_compact", energy=e, e_atom=ea, forces=f, positions=pos, n_iter=it, n_eval=ev, stop=why)
    lockstep, dispatched = eng.last_relax_counts   # (in clear, not hashed: dispatched < lockstep x chains shows the compaction)
    OUT["relax_cg_compact"]["relax_counts"] = {"lockstep": lockstep, "dispatched": dispatched, "chains": len(structs)}
    del os.environ["VSSR_CG_FUSED"], os.environ["VSSR_RELAX_COMPACT"]
    for opt in ("FIRE", "BFGS"):
        eng.upload(structs)
        out = eng.relax(opt, fixed=fixed, max_steps=30, fmax=0.01, want=1 | 2 | 16, record_interval=3)
        t = out["traj"]
        record(f"traj_{opt.lower()}", n_records=t["n_records"], pos=t["positions"], forces=t["forces"], energy=t["energies"],
               positions=out["positions"], n_steps=out["n_steps"], converged=out["converged"])


def flat(v):
    return np.concatenate([np.ravel(x) for x in v]) if isinstance(v, list) else v


def drivers(eng, prefix, tight, a, b, box, masses_of, resident):
    """Every driver beyond CG / FIRE / BFGS on one handle.  a, b: two structures (T, X, cell, pbc) of different positions (and, on
    the GaN handle, sizes); box: a fully periodic one; masses_of(T): amu per atom."""
    from surface_sampling_amd import backend

    def case(name, structs, call):
        if tight:
            eng.debug_capacity(slots_per_atom=1, tight=1)
        eng.upload(structs)
        try:
            out = call(structs)
        except backend.BackendError as err:   # (in clear: the same refusal from both builds is a record too)
            OUT[f"{prefix}_{name}"] = {"error": str(err)}
            return
        record(f"{prefix}_{name}", relax_counts=np.array(eng.last_relax_counts, np.int64), **{k: flat(v) for k, v in out.items()})
        OUT[f"{prefix}_{name}"]["regrows"] = eng.debug_capacity()   # (in clear: > 0 shows that a *_tight case did regrow)

    def held(structs):
        return np.concatenate([np.arange(len(s[0])) % 5 == 0 for s in structs]).astype(np.uint8)

    def masses(structs):
        return np.concatenate([masses_of(s[0]) for s in structs])

    def moved(s, k, n):   # image k of n on a straight line from s to a displaced copy of it
        d = np.random.default_rng(len(s[0])).normal(0, 0.08, s[1].shape)
        return (s[0], s[1] + d * k / (n - 1), s[2], s[3])

    def results(out):   # with the static results the driver left on the device
        if hasattr(eng, "results_f64"):
            e, ea, f = eng.results_f64()
            return dict(out, dev_energy=e, dev_e_atom=ea, dev_forces=f)
        res = eng.download()
        return dict(out, dev_energy=res["energy_f64"], dev_forces=res["forces"], dev_energy_std=res["energy_std"])

    case("bfgsls", [a, b], lambda S: results(eng.relax_bfgs_linesearch(fixed=held(S), max_steps=6, fmax=0.01)))
    for driver in ("lockstep", "resident") if resident else ("lockstep",):
        for thermostat in ("nve", "langevin"):
            def md(S):
                eng.draw_velocities(masses(S), 300.0, seed=5, fixed=held(S))
                return eng.md(masses(S), 6, 1.0, thermostat=thermostat, temperature=300.0, friction=0.01, seed=9, fixed=held(S),
                              thermo_interval=2, driver=driver)
            case(f"md_{driver}_{thermostat}", [a, b], md)
    case("vib", [a, a, b], lambda S: eng.vibrations(masses(S), vib=np.concatenate([np.arange(len(s[0])) < 4 for s in S]), n_rep=[2, 1],
                                                     temperature=300.0, return_hessian=True, return_modes=True))
    bands = [moved(a, k, 3) for k in range(3)] + [moved(b, k, 4) for k in range(4)]
    case("neb", bands, lambda S: results(eng.neb([3, 4], fixed=held(S), climb=True, max_steps=5)))
    case("dimer", [a, a, b, b], lambda S: results(eng.dimer(fixed=held(S), seed=3, max_steps=4)))
    case("cell_hydrostatic", [box], lambda S: results(eng.relax_cell(hydrostatic_strain=True, max_steps=5)))
    case("cell_slab", [a, b], lambda S: results(eng.relax_cell(fixed=held(S), mask=(1, 1, 0, 0, 0, 1), max_steps=5)))


def painn_relaxations():
    """The fp32 force path of the lock-step drivers: a PaiNN ensemble, two chains, different FixAtoms masks."""
    from surface_sampling_amd import backend

    blobs = [np.fromfile(os.path.join(GOLDEN, "weights", f"SrTiO3_painn_model0{m}.f32"), dtype="<f4") for m in (1, 2, 3)]
    S = np.load(os.path.join(GOLDEN, "structures.npz"))
    k = "SrTiO3_2x2_pristine"
    Z, X, cell, pbc = S[f"{k}.numbers"], S[f"{k}.positions"], S[f"{k}.cell"], S[f"{k}.pbc"]
    rng = np.random.default_rng(17)
    chains = [(Z, X + rng.normal(0, 0.03, X.shape), cell, pbc) for _ in range(2)]
    mask = np.concatenate([X[:, 2] < X[:, 2].min() + 2.0, np.arange(len(Z)) % 4 == 0]).astype(np.uint8)
    eng = backend.PainnEngine(blobs, device=0)
    for opt in ("FIRE", "BFGS"):
        eng.upload(chains)
        out = eng.relax(opt, fixed=mask, max_steps=6, fmax=0.01)
        res = eng.download()
        record(f"painn_{opt.lower()}", positions=out["positions"], n_steps=out["n_steps"], converged=out["converged"],
               energy=res["energy"], forces=res["forces"], energy_std=res["energy_std"])
    amu = {38: 87.62, 22: 47.867, 8: 15.999}
    drivers(eng, "painn", False, chains[0], chains[1], chains[0], lambda T: np.array([amu[int(z)] for z in T]), resident=False)
    eng.close()


def main():
    import eam_alloy_oracle as ao
    import pair_oracle as po
    import sw_oracle as so
    from conftest import synthetic_tersoff
    from surface_sampling_amd import backend, eam, pair

    with open(os.path.join(GOLDEN, "GaN_tersoff_params.json")) as fh:
        gan_params = np.array(json.load(fh)["params_ijk"], dtype=np.float64)
    gan = gan_batch()
    m = pair.parse(po.ROCKSALT_COMMANDS, 2)
    Tr, Xr, Cr = po.rocksalt(5.64)
    rep = np.array([[x, y, z] for x in range(2) for y in range(2) for z in range(2)], float) * 5.64
    rock = (np.tile(Tr, 8), (Xr[None] + rep[:, None]).reshape(-1, 3) + np.random.default_rng(21).normal(0, 0.05, (64, 3)), Cr * 2,
            np.ones(3, np.uint8))
    for tag, tight in (("", False), ("_tight", True)):
        eng = backend.TersoffEngine(gan_params, device=0)
        single_point("tersoff_gan" + tag, eng, gan, tight)
        relaxations(eng, gan, tag, tight)
        if not tight:
            relaxations_beyond(eng, gan)
        drivers(eng, "gan" + tag, tight, gan[1], gan[0], gan[2], lambda T: np.where(np.asarray(T) == 0, 69.723, 14.007), resident=True)
        eng.close()
        eng = backend.PairEngine(m, device=0)
        single_point("pair_rocksalt" + tag, eng, [rock], tight)
        eng.close()
    eng = backend.PairEngine(m, device=0)   # the lock-step drivers of a handle the chain-resident minimiser does not serve
    eng.debug_capacity(slots_per_atom=1, tight=1)
    e, ea, f, pos, it, ev, why = eng.relax_cg_f64([rock], max_iter=5, etol=0.0, ftol=1e-4)
    record("relax_cg_pair_tight", energy=e, e_atom=ea, forces=f, positions=pos, n_iter=it, n_eval=ev, stop=why)
    eng.close()

    eng = backend.TersoffEngine(synthetic_tersoff(5, 2), device=0)
    single_point("tersoff_5species", eng, [so.dense_box(n=30, box=8.0, min_dist=1.9, seed=5, nt=5)])
    eng.close()

    Z, X, Cl, pbc, _ = so.si_slab()
    eng = backend.SWEngine(so.si_params(), device=0)
    single_point("sw_si111", eng, [(np.zeros(len(Z), np.int32), X, Cl, pbc.astype(np.uint8))])
    eng.close()
    eng = backend.SWEngine(so.three_species()[1], device=0)
    single_point("sw_3species", eng, [so.dense_box(nt=3, seed=3)])
    eng.close()

    cu, au = eam.read_funcfl(os.path.join(GOLDEN, "Cu_u3.eam")), eam.read_funcfl(os.path.join(GOLDEN, "Au_u3.eam"))
    slabs = [with_adatoms("cu100", 3), with_adatoms("au110", 2)]
    one = [(np.zeros(len(x), np.int32), x, c, p) for x, c, p in slabs]
    two = [(ao.random_alloy(x, 0.4, 7 + k), x, c, p) for k, (x, c, p) in enumerate(slabs)]
    eng = backend.EAMEngine(cu, device=0)
    single_point("eam_funcfl", eng, one)
    eng.close()
    eng = backend.EAMEngine(eam.tables_from_setfl(ao.cuau_setfl(cu, au), ["Cu", "Au"]), device=0)
    single_point("eam_alloy", eng, two)
    eng.close()
    eng = backend.EAMEngine(eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au, (0.7, 1.3))), fs=True), ["Cu", "Au"]),
                            device=0)
    single_point("eam_fs", eng, two)
    eng.close()
    painn_relaxations()
    print(json.dumps(OUT, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
