"""PaiNN configurations beyond the shipped one (three models, three blocks, cutoff 5.0 A, 100 embedding rows, readout 64, repulsion
on with p = 12 and sigma = 1.5): model builders, structures, the case table and the acceptance rule shared by
tests/test_painn_config_cpu.py (pins the table with the oracle alone) and tests/test_gpu_painn_config.py (the device).

Every model is made from the shipped SrTiO3 blobs (layout: include/vssr_eval.h / checkpoint.painn_blob_shapes); every structure
has 60 .. 76 atoms.  The oracle's own fp32-against-fp64 deviation of every case is checked by the CPU file: only the cases named in
BEYOND_CONTRACT (cutoff 6.0 A: 1.2e-4 eV / 3.5e-4 eV/A) miss the contract of tests/test_gpu_parity.py on their own.
"""
from dataclasses import dataclass, replace

import numpy as np

from painn_shapes import SRC, reshape_blob

E_TOL, F_TOL, STD_TOL = 1e-4, 2e-4, 2e-4      # the contract of tests/test_gpu_parity.py
SHIPPED = {"order": (0, 1, 2), "cutoff": 5.0, "excl_vol": True, "p": 12, "sigma": 1.5, "H": 64, "n_embed": 100, "M": 3}


# ---- model builders ------------------------------------------------------------------------------------------------------------
def _hp(num_conv=3, readout_hidden=64, n_embed=100):
    return {**SRC, "num_conv": num_conv, "readout_hidden": readout_hidden, "n_embed": n_embed}


def _assemble(fields, hp):
    from surface_sampling_amd import checkpoint

    parts = []
    for k, shp in checkpoint.painn_blob_shapes(hp).items():
        assert fields[k].shape == shp, (k, fields[k].shape, shp)
        parts.append(np.asarray(fields[k], np.float32).reshape(-1))
    return np.ascontiguousarray(np.concatenate(parts), dtype="<f4")


def relayer(blob, order, readout_hidden=64, n_embed=100):
    """A model whose block l is block order[l] of ``blob`` (a three-block model), message and update parts together; embedding and
    readout unchanged."""
    from surface_sampling_amd import checkpoint

    src = checkpoint.blob_to_fields(np.asarray(blob, np.float32), _hp(3, readout_hidden, n_embed))
    out = {k: v for k, v in src.items() if not k.startswith(("msg", "upd"))}
    for l, o in enumerate(order):
        for k, v in src.items():
            if k.startswith((f"msg{o}.", f"upd{o}.")):
                out[k[:3] + str(l) + k[4:]] = v
    return _assemble(out, _hp(len(order), readout_hidden, n_embed))


def cut_embed(blob, n_embed, num_conv=3, readout_hidden=64):
    """The model with the first ``n_embed`` rows of its embedding table."""
    from surface_sampling_amd import checkpoint

    src = dict(checkpoint.blob_to_fields(np.asarray(blob, np.float32), _hp(num_conv, readout_hidden, 100)))
    src["embed"] = src["embed"][:n_embed]
    return _assemble(src, _hp(num_conv, readout_hidden, n_embed))


def perturbed_ensemble(blobs, M):
    """M distinct models: blobs[m % 3] * (1 + 0.02 N(0, 1)), seeded per m."""
    out = []
    for m in range(M):
        b = np.asarray(blobs[m % len(blobs)], np.float32)
        out.append((b * (1.0 + 0.02 * np.random.default_rng(m).standard_normal(b.size))).astype("<f4"))
    return out


# ---- structures ----------------------------------------------------------------------------------------------------------------
def structure(golden, name):
    from surface_sampling_amd import structures

    if name == "base":
        return golden.structure("SrTiO3_2x2_pristine")
    if name == "O40":
        return golden.structure("O40Sr16Ti12")
    if name.startswith("syn"):     # syn4: an adatom with forces near 94 eV/A, so the repulsion matters
        return structures.synth_chain(golden.structure("SrTiO3_2x2_pristine"), int(name[3:]))
    raise KeyError(name)


def arrays(s):
    return (s.numbers, s.positions, s.cell, s.pbc)


# ---- the case table ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    axis: str                       # the parameter the case moves away from the shipped value
    structs: tuple
    order: tuple = (0, 1, 2)
    M: int = 3
    cutoff: float = 5.0
    excl_vol: bool = True
    p: int = 12
    sigma: float = 1.5
    H: int = 64
    n_embed: int = 100

    @property
    def L(self):
        return len(self.order)

    def blobs(self, golden):
        blobs = list(golden.blobs[:self.M]) if self.M <= 3 else perturbed_ensemble(golden.blobs, self.M)
        out = []
        for m, b in enumerate(blobs):
            if self.H != 64:
                b, _ = reshape_blob(b, 128, 20, readout_hidden=self.H, seed=m)
            if self.order != (0, 1, 2):
                b = relayer(b, self.order, self.H)
            if self.n_embed != 100:
                b = cut_embed(b, self.n_embed, self.L, self.H)
            out.append(b)
        return out

    def engine_hp(self):
        return {"num_conv": self.L, "readout_hidden": self.H, "n_embed": self.n_embed, "excl_vol": self.excl_vol,
                "V_ex_power": self.p, "V_ex_sigma": self.sigma}

    def oracle_hp(self, oracle_mod):
        return oracle_mod.default_hparams(num_conv=self.L, readout_hidden=self.H, n_embed=self.n_embed, excl_vol=int(self.excl_vol),
                                          excl_power=self.p, cutoff=self.cutoff, excl_sigma=self.sigma)

    def offset(self, golden):
        table, const = golden.offset_table()
        return np.ascontiguousarray(table[:self.n_embed]), const

    def shipped(self):
        """The same case with its axis back at the shipped value (what a device that ignored the parameter would compute)."""
        back = {"depth": {"order": (0, 1, 2)}, "models": {"M": 3}, "cutoff": {"cutoff": 5.0},
                "repulsion": {"excl_vol": True, "p": 12, "sigma": 1.5}, "embed": {"n_embed": 100}, "readout": {"H": 64}}[self.axis]
        return replace(self, id=self.id + "@shipped", **back)


def _cases():
    slabs, syn = ("base", "O40"), ("syn4",)
    c = []
    for order in ((2,), (0,), (0, 2), (1, 2), (0, 1, 1, 2)):
        c.append(Case(f"depth{len(order)}-" + "".join(map(str, order)), "depth", slabs, order=order))
    for M in (1, 2, 5, 8):
        c.append(Case(f"models-{M}", "models", syn, M=M))
    for rc in (4.0, 4.5, 5.5, 6.0):
        c.append(Case(f"cutoff-{rc}", "cutoff", ("O40", "syn4"), cutoff=rc))
    c.append(Case("repulsion-off", "repulsion", syn, excl_vol=False))
    c.append(Case("repulsion-off-p0", "repulsion", syn, excl_vol=False, p=0))
    for p, sg in ((1, 1.5), (2, 1.0), (7, 1.5), (13, 1.2), (6, 2.5), (33, 1.6)):
        c.append(Case(f"repulsion-p{p}-s{sg}", "repulsion", slabs, p=p, sigma=sg))
    c.append(Case("repulsion-p64-s1.5", "repulsion", syn, p=64, sigma=1.5))
    c.append(Case("embed-39", "embed", slabs, n_embed=39))          # Sr, Z = 38, is the last row
    for H in (1, 40, 128):
        c.append(Case(f"readout-{H}-depth3", "readout", syn, H=H))
    for H in (1, 32, 40, 128):
        c.append(Case(f"readout-{H}-depth1", "readout", syn, H=H, order=(2,)))
    # beyond the table: the unfused reverse path (H = 32) at depths 2 and 4, and batches that mix a slab with a chain of another
    # slice class (tests/test_gpu_painn_config.py moves the 72-atom chain there through the class knobs) at depths 2 and 4
    c.append(Case("readout-32-depth2", "readout", syn, H=32, order=(0, 2)))
    c.append(Case("readout-32-depth4", "readout", syn, H=32, order=(0, 1, 1, 2)))
    # ... the stand-alone readout (H != 64) with the repulsion off: the one kernel that is handed the repulsion buffer all the same
    c.append(Case("repulsion-off-p0-readout-32", "repulsion", syn, excl_vol=False, p=0, H=32))
    c.append(Case("depth2-02-mixed", "depth", ("base", "syn4"), order=(0, 2)))
    c.append(Case("depth4-0112-mixed", "depth", ("base", "syn4"), order=(0, 1, 1, 2)))
    return c


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
BEYOND_CONTRACT = ["cutoff-6.0"]      # the oracle's own fp32 run misses the contract there (tests/test_painn_config_cpu.py proves: only there)

DEPTH_CASES = [c for c in CASES if c.axis == "depth" and not c.id.endswith("-mixed")]
MIXED_CASES = [c for c in CASES if c.id.endswith("-mixed")]
BOTH_PATH_CASES = [c for c in CASES if c.axis in ("models", "cutoff", "repulsion")]


# ---- references (computed once, shared) ------------------------------------------------------------------------------------------
_REF = {}


def reference(golden, oracle_mod, case, name, bits=64):
    """The oracle's ensemble result of one structure of a case; computed once per session and never changed."""
    key = (case.id, name, bits)
    if key not in _REF:
        s = structure(golden, name)
        table, const = case.offset(golden)
        r = oracle_mod.ensemble(case.blobs(golden), s.numbers, s.positions, s.cell, s.pbc, bits, table, const, hp=case.oracle_hp(oracle_mod))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def deviation(a, ref):
    """(|dE|, max |dF|, |d energy_std|, max |d forces_std|) of two ensemble results."""
    return (abs(a["energy"] - ref["energy"]), float(np.abs(a["forces"] - ref["forces"]).max()),
            abs(a["energy_std"] - ref["energy_std"]), float(np.abs(a["forces_std"] - ref["forces_std"]).max()))


# ---- the acceptance rule ---------------------------------------------------------------------------------------------------------
def check(golden, oracle_mod, blobs, ohp, s, e, f, std, tag="", fstd=None, beyond=True, refs=None):
    """Device results of one structure against the fp64 oracle; returns (dE, dF, dstd).  Accepted: inside the contract, or -- with
    ``beyond`` -- within twice the oracle's own fp32 deviation on the same structure.  ``fstd``: also forces_std, at F_TOL.
    ``refs``: (fp64, fp32) oracle results where the caller has them already."""
    if refs is None:
        table, const = golden.offset_table()
        refs = [oracle_mod.ensemble(blobs, s.numbers, s.positions, s.cell, s.pbc, bits, table, const, hp=ohp) for bits in (64, 32)]
    ref, r32 = refs
    de, df, ds = abs(e - ref["energy"]), float(np.abs(f - ref["forces"]).max()) if len(f) else 0.0, abs(std - ref["energy_std"])
    de32 = abs(r32["energy"] - ref["energy"])
    df32 = float(np.abs(r32["forces"] - ref["forces"]).max()) if len(f) else 0.0
    ds32 = abs(r32["energy_std"] - ref["energy_std"])
    line = (f"deviation from the fp64 oracle {tag} N={len(s.numbers)}: device dE {de:.2e} dF {df:.2e} dstd {ds:.2e} | "
            f"oracle fp32 dE {de32:.2e} dF {df32:.2e} dstd {ds32:.2e}")
    dfs = dfs32 = 0.0
    if fstd is not None:
        dfs = float(np.abs(fstd - ref["forces_std"]).max())
        dfs32 = float(np.abs(r32["forces_std"] - ref["forces_std"]).max())
        line += f" | forces_std device {dfs:.2e} oracle fp32 {dfs32:.2e}"
    print(line)
    if de <= E_TOL and df <= F_TOL and ds <= STD_TOL and dfs <= F_TOL:
        return de, df, ds
    assert beyond, (tag, de, df, ds, dfs)
    assert de <= max(E_TOL, 2 * de32), (tag, de, de32)
    assert df <= max(F_TOL, 2 * df32), (tag, df, df32)
    assert ds <= max(STD_TOL, 2 * ds32), (tag, ds, ds32)
    assert dfs <= max(F_TOL, 2 * dfs32), (tag, dfs, dfs32)
    return de, df, ds
