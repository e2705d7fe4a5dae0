"""Test models of other PaiNN shapes, made from the shipped SrTiO3 weights.

Every matrix is cut to (or padded with small seeded noise up to) the new feature width F, section by section: the 3F rows of
W2 / b2 / Wd / bd / W4 / b4 keep their a / b / c split and the 2F columns of W3 their [s ; |V v|] split.  The radial filter
keeps its first R columns (or is padded), the message / update blocks the first num_conv layers (a fourth repeats the
third).  The energies are not
physical, the weights keep a realistic scale.
"""

import io
import sys
import types

import numpy as np

SRC = {"feat_dim": 128, "n_rbf": 20, "num_conv": 3, "readout_hidden": 64, "n_embed": 100}


def _fit(a, axis, sections, new, rng):
    """Resize ``axis`` of ``a`` (``sections`` equal parts) to ``sections`` parts of ``new`` entries each."""
    parts = np.split(a, sections, axis=axis)
    out = []
    for p in parts:
        n = p.shape[axis]
        if new <= n:
            out.append(np.take(p, np.arange(new), axis=axis))
        else:
            shape = list(p.shape)
            shape[axis] = new - n
            scale = float(np.std(p)) if p.size > 1 else 0.05
            out.append(np.concatenate([p, rng.normal(0.0, 0.5 * scale, shape).astype(np.float32)], axis=axis))
    return np.concatenate(out, axis=axis)


def reshape_blob(blob, F, R, num_conv=3, readout_hidden=64, seed=0):
    """The canonical blob of a shipped model cut / padded to (F, R, num_conv, readout_hidden)."""
    from surface_sampling_amd import checkpoint

    rng = np.random.default_rng(seed)
    src = checkpoint.blob_to_fields(np.asarray(blob, np.float32), SRC)
    hp = {**SRC, "feat_dim": F, "n_rbf": R, "num_conv": num_conv, "readout_hidden": readout_hidden}
    out = {}
    out["embed"] = _fit(src["embed"], 1, 1, F, rng)
    for l in range(num_conv):
        g = lambda k: src[k.format(l=min(l, SRC["num_conv"] - 1))]   # noqa: E731  (a fourth block repeats the third)
        out[f"msg{l}.W1"] = _fit(_fit(g("msg{l}.W1"), 0, 1, F, rng), 1, 1, F, rng)
        out[f"msg{l}.b1"] = _fit(g("msg{l}.b1"), 0, 1, F, rng)
        out[f"msg{l}.W2"] = _fit(_fit(g("msg{l}.W2"), 0, 3, F, rng), 1, 1, F, rng)
        out[f"msg{l}.b2"] = _fit(g("msg{l}.b2"), 0, 3, F, rng)
        out[f"msg{l}.Wd"] = _fit(_fit(g("msg{l}.Wd"), 0, 3, F, rng), 1, 1, R, rng)
        out[f"msg{l}.bd"] = _fit(g("msg{l}.bd"), 0, 3, F, rng)
        out[f"upd{l}.U"] = _fit(_fit(g("upd{l}.U"), 0, 1, F, rng), 1, 1, F, rng)
        out[f"upd{l}.V"] = _fit(_fit(g("upd{l}.V"), 0, 1, F, rng), 1, 1, F, rng)
        out[f"upd{l}.W3"] = _fit(_fit(g("upd{l}.W3"), 0, 1, F, rng), 1, 2, F, rng)
        out[f"upd{l}.b3"] = _fit(g("upd{l}.b3"), 0, 1, F, rng)
        out[f"upd{l}.W4"] = _fit(_fit(g("upd{l}.W4"), 0, 3, F, rng), 1, 1, F, rng)
        out[f"upd{l}.b4"] = _fit(g("upd{l}.b4"), 0, 3, F, rng)
    out["readout.W5"] = _fit(_fit(src["readout.W5"], 0, 1, readout_hidden, rng), 1, 1, F, rng)
    out["readout.b5"] = _fit(src["readout.b5"], 0, 1, readout_hidden, rng)
    out["readout.w6"] = _fit(src["readout.w6"], 1, 1, readout_hidden, rng)
    out["readout.b6"] = src["readout.b6"].copy()
    shapes = checkpoint.painn_blob_shapes(hp)
    parts = []
    for k, shp in shapes.items():
        assert out[k].shape == shp, (k, out[k].shape, shp)
        parts.append(out[k].reshape(-1))
    return np.ascontiguousarray(np.concatenate(parts), dtype="<f4"), hp


def reshape_ensemble(blobs, F, R, num_conv=3, readout_hidden=64):
    res = [reshape_blob(b, F, R, num_conv, readout_hidden, seed=m) for m, b in enumerate(blobs)]
    return [b for b, _ in res], res[0][1]


def checkpoint_bytes(blob, hp, cutoff=5.0):
    """``torch.save`` of a whole module under ``nff.*`` class names holding ``blob`` (the reference's ``best_model`` format)."""
    import torch

    from surface_sampling_amd import checkpoint

    names = ("nff", "nff.nn", "nff.nn.models", "nff.nn.models.painn", "nff.nn.modules", "nff.nn.modules.painn")
    mods = {n: types.ModuleType(n) for n in names}

    class Painn(torch.nn.Module):
        pass

    class Block(torch.nn.Module):
        pass

    Painn.__module__, Painn.__qualname__ = "nff.nn.models.painn", "Painn"
    Block.__module__, Block.__qualname__ = "nff.nn.modules.painn", "Block"
    mods["nff.nn.models.painn"].Painn = Painn
    mods["nff.nn.modules.painn"].Block = Block
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        fields = checkpoint.blob_to_fields(np.asarray(blob, np.float32), hp)
        top = Painn()
        for field, key in checkpoint.painn_blob_order(hp["num_conv"]):
            parts = key.split(".")
            node = top
            for part in parts[:-1]:
                if part not in node._modules:
                    node.add_module(part, Block())
                node = node._modules[part]
            node.register_parameter(parts[-1], torch.nn.Parameter(torch.from_numpy(np.array(fields[field], dtype=np.float32))))
        top.excl_vol, top.power, top.sigma, top.cutoff = True, 12, 1.5, float(cutoff)
        buf = io.BytesIO()
        torch.save(top, buf)
        return buf.getvalue()
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def state_dict_of(blob, hp):
    """{state-dict key: array} of a canonical blob."""
    from surface_sampling_amd import checkpoint

    fields = checkpoint.blob_to_fields(np.asarray(blob, np.float32), hp)
    return {key: np.array(fields[field]) for field, key in checkpoint.painn_blob_order(hp["num_conv"])}
