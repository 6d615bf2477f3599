"""Host side of the predictor (sgdml_amd.predict.GDMLPredict, sgdml_amd.model.test_errors):
model loading, shape normalisation of the geometries, the refusals, the error arithmetic of
the reference's test step (cli.py:855-865, 1217-1245) and the C ABI's argument checks.  CPU
only: nothing here creates a device context."""
import numpy as np
import pytest

from sgdml_amd import model as mdl
from sgdml_amd import predict as prd


def model_of(golden_dir):
    f = np.load(golden_dir / "sgdml_model_ethanol_n621.npz", allow_pickle=False)
    return {k[len("model__"):]: f[k] for k in f.files if k.startswith("model__")}


def test_exported_from_the_package():
    import sgdml_amd

    assert sgdml_amd.GDMLPredict is prd.GDMLPredict


def test_load_from_dict(golden_dir):
    m = model_of(golden_dir)
    a = prd.load_model_arrays(m)
    assert a["R_desc"].shape == (23, 36) and a["R_desc"].flags.c_contiguous
    np.testing.assert_array_equal(a["R_desc"], m["R_desc"].T)      # stored D x M
    np.testing.assert_array_equal(a["R_d_desc_alpha"], m["R_d_desc_alpha"])
    assert a["perms"].dtype == np.int32 and a["perms"].shape == (1, 9)
    assert a["sig"] == 10.0 and isinstance(a["sig"], float)
    assert a["std"] == float(m["std"]) and a["c"] == float(m["c"])
    m.pop("std")                                                   # predict.py:313
    assert prd.load_model_arrays(m)["std"] == 1.0


def test_load_from_npz_path_with_0d_and_pickled_entries(golden_dir, tmp_path):
    """A file as store_model / the reference write it: scalars come back as 0-d arrays, and
    dict / None fields are pickled -- they are never read."""
    m = model_of(golden_dir)
    m.update(f_err={"mae": np.nan, "rmse": np.nan}, md5_test=None, interact_cut_off=None)
    path = tmp_path / "model.npz"
    np.savez_compressed(path, **m)
    back = np.load(path, allow_pickle=True)
    assert back["sig"].shape == () and back["c"].shape == ()
    a, b = prd.load_model_arrays(path), prd.load_model_arrays(str(path))
    ref = prd.load_model_arrays(model_of(golden_dir))
    for key in ref:
        np.testing.assert_array_equal(a[key], ref[key])
        np.testing.assert_array_equal(b[key], ref[key])
    with np.load(path, allow_pickle=False) as opened:              # an open np.load result
        c = prd.load_model_arrays(opened)
    np.testing.assert_array_equal(c["R_desc"], ref["R_desc"])


def test_refusals(golden_dir):
    m = model_of(golden_dir)
    with pytest.raises(NotImplementedError):
        prd.load_model_arrays(dict(m, lattice=np.eye(3)))
    with pytest.raises(NotImplementedError):
        prd.load_model_arrays(dict(m, alphas_E=np.zeros(23)))
    with pytest.raises(NotImplementedError):
        prd.load_model_arrays(dict(m, interact_cut_off=5.0))
    with pytest.raises(NotImplementedError):
        prd.GDMLPredict(dict(m, lattice=np.eye(3)))                # before any device is touched
    with pytest.raises(ValueError):
        prd.load_model_arrays(dict(m, R_desc=m["R_desc"][:-1]))    # D does not match z
    with pytest.raises(ValueError):
        prd.load_model_arrays(dict(m, R_d_desc_alpha=m["R_d_desc_alpha"][:-1]))
    with pytest.raises(ValueError):
        prd.load_model_arrays(dict(m, perms=np.arange(8)[None, :]))
    with pytest.raises(ValueError):
        prd.load_model_arrays(dict(m, perms=np.zeros((1, 9), dtype=int)))
    with pytest.raises(ValueError):
        prd.load_model_arrays(dict(m, sig=np.array([10.0, 11.0])))
    with pytest.raises(ValueError):
        prd.load_model_arrays(dict(m, type=np.array("t")))
    with pytest.raises(ValueError):
        prd.load_model_arrays({k: v for k, v in m.items() if k != "c"})


def test_geometry_shapes():
    rng = np.random.default_rng(0)
    R = rng.standard_normal((5, 9, 3))
    for given in (R, R.reshape(5, 27), R.reshape(5, 27)[:, ::1].copy(order="F")):
        out = prd.normalize_geometries(given, 9)
        assert out.shape == (5, 9, 3) and out.flags.c_contiguous
        np.testing.assert_array_equal(out, R)
    for one in (R[0], R[0].ravel()):
        np.testing.assert_array_equal(prd.normalize_geometries(one, 9), R[:1])
    assert prd.normalize_geometries(np.empty((0, 27)), 9).shape == (0, 9, 3)
    # 3 atoms: a 3 x 3 array is one geometry (n x 3), 1 x 9 and 2 x 9 are batches
    assert prd.normalize_geometries(np.zeros((3, 3)), 3).shape == (1, 3, 3)
    assert prd.normalize_geometries(np.zeros((2, 9)), 3).shape == (2, 3, 3)
    for bad in (np.zeros(26), np.zeros((5, 26)), np.zeros((5, 8, 3)), np.zeros((2, 5, 9, 3))):
        with pytest.raises(ValueError):
            prd.normalize_geometries(bad, 9)


def test_split_blocks():
    assert prd.split_blocks(70, 3) == [(0, 24), (24, 48), (48, 70)]
    assert prd.split_blocks(2, 3) == [(0, 1), (1, 2), (2, 2)]     # one empty block
    assert prd.split_blocks(0, 2) == [(0, 0), (0, 0)]
    for Q, parts in ((7, 4), (64, 5), (1, 1)):
        b = prd.split_blocks(Q, parts)
        assert b[0][0] == 0 and b[-1][1] == Q and all(x[1] == y[0] for x, y in zip(b, b[1:]))


def test_tile_queries_per_workgroup():
    assert [prd.tile_queries_per_workgroup(D) for D in (3, 36, 37, 72, 112, 224, 288)] == \
        [64, 64, 32, 32, 32, 16, 16]
    with pytest.raises(ValueError):
        prd.tile_queries_per_workgroup(289)


def test_prediction_errors_arithmetic():
    """cli.py:855-865 over one batch: mae = sum |err| / (3 n) / Q, rmse = sqrt(sum err^2 / (3 n) / Q)."""
    F = np.zeros((2, 6))
    F_pred = np.array([[1.0, -1.0, 0.0, 0.0, 2.0, 0.0], [0.0, 0.0, 0.0, -2.0, 0.0, 0.0]])
    E, E_pred = np.array([1.0, 5.0]), np.array([0.0, 2.0])
    out = mdl.prediction_errors(E_pred, F_pred, F, E)
    assert out["n_test"] == 2
    assert out["f_err"] == {"mae": 6.0 / 12.0, "rmse": float(np.sqrt(10.0 / 12.0))}
    assert out["e_err"] == {"mae": 2.0, "rmse": float(np.sqrt(5.0))}
    out = mdl.prediction_errors(E_pred, F_pred.reshape(2, 2, 3), F.reshape(2, 2, 3))
    assert out["e_err"] is None and out["f_err"]["mae"] == 0.5
    with pytest.raises(ValueError):
        mdl.prediction_errors(E_pred, F_pred, F[:1])
    with pytest.raises(ValueError):
        mdl.prediction_errors(E_pred, F_pred, F, E[:1])


def test_abi_rejects_null_context_and_bad_calls():
    from sgdml_amd import _native

    lib = _native.load_library()
    assert lib.mlff_predict(None, None, 1, None, None) == _native.MLFF_ERR_ARG
    assert lib.mlff_predict_set_model(None, None, None, 1, 2, None, 1, 10.0, 1.0, 0.0) == \
        _native.MLFF_ERR_ARG
    assert lib.mlff_predict_info(None, None, None, None, None) == _native.MLFF_ERR_ARG


def test_model_docstring_lists_the_predictor():
    assert "test_errors" in mdl.__doc__ and "GDMLPredict" in mdl.__doc__
