"""CPU: the Python side of PaiNN models of other widths -- shape inference from checkpoint tensors (``hparams="auto"``),
``params.json`` cross-checks, the blob layout for every shape, and the unchanged 128 / 20 loader."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from painn_shapes import checkpoint_bytes, reshape_blob, state_dict_of

SHAPES = [(16, 8, 1, 32), (64, 16, 2, 64), (96, 20, 3, 16), (256, 32, 4, 128), (128, 20, 3, 64)]


def _golden_blob(m=1):
    return np.fromfile(os.path.join(GOLDEN, "weights", f"SrTiO3_painn_model0{m}.f32"), dtype="<f4")


@pytest.mark.parametrize("F,R,L,H", SHAPES)
def test_infer_hparams_reads_the_shapes_from_the_tensors(F, R, L, H):
    from surface_sampling_amd import checkpoint

    blob, hp = reshape_blob(_golden_blob(), F, R, L, H)
    got = checkpoint.infer_hparams(state_dict_of(blob, hp))
    for k in ("feat_dim", "n_rbf", "num_conv", "readout_hidden", "n_embed"):
        assert got[k] == hp[k], k
    assert got["cutoff"] == checkpoint.DEFAULT_HPARAMS["cutoff"]


def test_infer_hparams_rejects_a_foreign_state_dict():
    from surface_sampling_amd import checkpoint

    with pytest.raises(ValueError, match="embed_block"):
        checkpoint.infer_hparams({"w": np.zeros((3, 3), np.float32)})


@pytest.mark.parametrize("F,R,L,H", SHAPES)
def test_blob_layout_round_trips_for_every_shape(F, R, L, H):
    from surface_sampling_amd import checkpoint

    blob, hp = reshape_blob(_golden_blob(), F, R, L, H)
    fields = checkpoint.blob_to_fields(blob, hp)
    assert fields["embed"].shape == (100, F) and fields["msg0.Wd"].shape == (3 * F, R)
    assert fields[f"upd{L - 1}.W3"].shape == (F, 2 * F) and fields["readout.W5"].shape == (H, F)
    sd = state_dict_of(blob, hp)
    assert np.array_equal(checkpoint.state_dict_to_blob(sd, hp), blob)
    with pytest.raises(ValueError):                      # another shape does not accept it
        checkpoint.blob_to_fields(blob, {**hp, "feat_dim": F + 16})


def test_reshaped_model_keeps_the_sections_of_the_shipped_weights():
    from surface_sampling_amd import checkpoint

    src = checkpoint.blob_to_fields(_golden_blob())
    blob, hp = reshape_blob(_golden_blob(), 64, 16)
    f = checkpoint.blob_to_fields(blob, hp)
    for s in range(3):   # a / b / c sections of the 3F rows
        assert np.array_equal(f["msg1.W2"][64 * s:64 * s + 64], src["msg1.W2"][128 * s:128 * s + 64, :64])
        assert np.array_equal(f["msg0.Wd"][64 * s:64 * s + 64], src["msg0.Wd"][128 * s:128 * s + 64, :16])
    assert np.array_equal(f["upd2.W3"][:, 64:], src["upd2.W3"][:64, 128:192])   # the |V v| half of [s ; |V v|]


@pytest.mark.parametrize("F,R,L,H", [(64, 16, 3, 64), (32, 12, 2, 32)])
def test_auto_loader_reads_checkpoint_and_params_json(tmp_path, F, R, L, H):
    pytest.importorskip("torch")
    from surface_sampling_amd import checkpoint

    blob, hp = reshape_blob(_golden_blob(), F, R, L, H)
    path = tmp_path / "best_model"
    path.write_bytes(checkpoint_bytes(blob, hp))
    got, ghp = checkpoint.load_painn_blob_auto(str(path))
    assert np.array_equal(got, blob) and ghp["feat_dim"] == F and ghp["n_rbf"] == R and ghp["num_conv"] == L
    (tmp_path / "params.json").write_text(json.dumps({"feat_dim": F, "n_rbf": R, "num_conv": L, "cutoff": 5.0,
                                                      "V_ex_power": 12, "V_ex_sigma": 1.5, "activation": "swish"}))
    got2, _ = checkpoint.load_painn_blob_auto(str(path))
    assert np.array_equal(got2, blob)


@pytest.mark.parametrize("bad,match", [({"feat_dim": 128}, "feat_dim"), ({"n_rbf": 20}, "n_rbf"), ({"num_conv": 4}, "num_conv"),
                                       ({"cutoff": 6.0}, "cutoff"), ({"V_ex_power": 6}, "power")])
def test_params_json_that_disagrees_raises(tmp_path, bad, match):
    pytest.importorskip("torch")
    from surface_sampling_amd import checkpoint

    blob, hp = reshape_blob(_golden_blob(), 64, 16)
    path = tmp_path / "best_model"
    path.write_bytes(checkpoint_bytes(blob, hp))
    (tmp_path / "params.json").write_text(json.dumps({"feat_dim": 64, "n_rbf": 16, "num_conv": 3, **bad}))
    with pytest.raises(ValueError, match=match):
        checkpoint.load_painn_blob_auto(str(path))


def test_auto_loader_refuses_a_raw_blob(tmp_path):
    from surface_sampling_amd import checkpoint

    p = tmp_path / "m.f32"
    _golden_blob().tofile(p)
    with pytest.raises(ValueError, match="auto"):
        checkpoint.load_painn_blob_auto(str(p))


def test_load_painn_blob_of_the_128_20_archive_is_unchanged(tmp_path):
    pytest.importorskip("torch")
    from surface_sampling_amd import checkpoint

    blob = _golden_blob()
    path = tmp_path / "best_model"
    path.write_bytes(checkpoint_bytes(blob, checkpoint.DEFAULT_HPARAMS))
    assert np.array_equal(checkpoint.load_painn_blob(str(path)), blob)
    assert np.array_equal(checkpoint.load_painn_blob(str(path), None), blob)
    got, hp = checkpoint.load_painn_blob_auto(str(path))
    assert np.array_equal(got, blob) and hp == {**checkpoint.DEFAULT_HPARAMS}
    # a model of another width never loads under the default shape
    b64, hp64 = reshape_blob(blob, 64, 16)
    p64 = tmp_path / "m64" / "best_model"
    p64.parent.mkdir()
    p64.write_bytes(checkpoint_bytes(b64, hp64))
    with pytest.raises(ValueError):
        checkpoint.load_painn_blob(str(p64))


def test_unsupported_shapes_are_refused_naming_the_accepted_set():
    """vssr_create checks the shape before it looks for a device."""
    from surface_sampling_amd import backend

    blob = _golden_blob()
    for hp in ({"feat_dim": 100}, {"n_rbf": 40}, {"feat_dim": 272}, {"n_rbf": 0}):
        with pytest.raises(backend.BackendError, match=r"multiple of 16 in 16\.\.256 and n_rbf in 1\.\.32"):
            backend.PainnEngine([blob], device=0, hparams=hp)


def test_auto_hparams_take_the_models_cutoff_and_refuse_another(tmp_path):
    """hparams="auto": without a cutoff argument the engine uses the models' own (module attribute or params.json); an
    explicit cutoff that differs raises instead of running the model at a radius it was not trained for."""
    pytest.importorskip("torch")
    from surface_sampling_amd.calculators import EnsembleNFFSurface

    blob, hp = reshape_blob(_golden_blob(), 64, 16)
    path = tmp_path / "best_model"
    path.write_bytes(checkpoint_bytes(blob, hp, cutoff=6.0))
    calc = EnsembleNFFSurface([str(path)], device="cuda:0", hparams="auto")
    assert calc.cutoff == 6.0 and calc.hparams["cutoff"] == 6.0
    assert EnsembleNFFSurface([str(path)], device="cuda:0", hparams="auto", cutoff=6.0).cutoff == 6.0
    with pytest.raises(ValueError, match="cutoff"):
        EnsembleNFFSurface([str(path)], device="cuda:0", hparams="auto", cutoff=5.0)
    (tmp_path / "params.json").write_text(json.dumps({"feat_dim": 64, "n_rbf": 16, "cutoff": 5.0}))
    with pytest.raises(ValueError, match="cutoff"):   # params.json and the module attribute disagree
        EnsembleNFFSurface([str(path)], device="cuda:0", hparams="auto")
    # without "auto" the default stays 5.0
    assert EnsembleNFFSurface([_golden_blob()], device="cuda:0").cutoff == 5.0


def test_general_path_isa_keeps_loads_out_of_mfma_blocks():
    """The general path's node GEMM (k_gen_gemm, painn_gen.hip) under the project's MFMA ISA rules (tools/check_mfma_loads.py):
    no load inside a dense MFMA block, no FLAT memory instructions.  Cross-compiles the file (no GPU needed)."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hip = os.path.join(root, "surface-sampling_amd", "csrc", "painn_gen.hip")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_mfma_loads.py"), hip], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = __import__("re").search(r"painn_gen\.hip: \d+ MFMA groups checked, (\d+) dense MFMA pairs, 0 violations", r.stdout)
    assert m and int(m.group(1)) >= 31, r.stdout     # the 32 MFMAs of a k-step form one dense block
