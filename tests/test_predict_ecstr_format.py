"""Host side of prediction with energy-constrained models (`alphas_E`):
sgdml_amd.predict.load_model_arrays(model, energy_constraints=True).  CPU only: nothing here
creates a device context."""
import numpy as np
import pytest

from sgdml_amd import predict as prd

M = 23


def model_of(golden_dir):
    f = np.load(golden_dir / "sgdml_model_ethanol_n621.npz", allow_pickle=False)
    return {k[len("model__"):]: f[k] for k in f.files if k.startswith("model__")}


def coefficients():
    return np.random.default_rng(7).standard_normal(M)


def test_returns_alphas_E(golden_dir):
    m = model_of(golden_dir)
    aE = coefficients()
    # given as a strided view: the loader returns a contiguous float64 array
    wide = np.zeros((M, 2))
    wide[:, 0] = aE
    a = prd.load_model_arrays(dict(m, alphas_E=wide[:, 0]), energy_constraints=True)
    assert a["alphas_E"].shape == (M,) and a["alphas_E"].dtype == np.float64
    assert a["alphas_E"].flags.c_contiguous
    assert np.array_equal(a["alphas_E"], aE)
    ref = prd.load_model_arrays(m)
    for key in ref:                                    # everything else as without the keyword
        np.testing.assert_array_equal(a[key], ref[key])
    assert sorted(a) == sorted(list(ref) + ["alphas_E"])


def test_none_without_the_key(golden_dir):
    a = prd.load_model_arrays(model_of(golden_dir), energy_constraints=True)
    assert "alphas_E" in a and a["alphas_E"] is None


@pytest.mark.parametrize("shape", [(M - 1,), (M, 2)])
def test_wrong_shape_is_a_value_error(golden_dir, shape):
    m = dict(model_of(golden_dir), alphas_E=np.zeros(shape))
    with pytest.raises(ValueError, match="alphas_E"):
        prd.load_model_arrays(m, energy_constraints=True)


def test_default_mode_still_refuses(golden_dir):
    m = dict(model_of(golden_dir), alphas_E=coefficients())
    with pytest.raises(NotImplementedError):
        prd.load_model_arrays(m)
    with pytest.raises(NotImplementedError):
        prd.load_model_arrays(m, energy_constraints=False)


def test_stored_model_loads_bit_for_bit(golden_dir, tmp_path):
    """A file as store_model writes it (np.savez_compressed, pickled dict / None fields that are
    never read), reopened by path and as an open np.load result."""
    aE = coefficients()
    m = dict(model_of(golden_dir), alphas_E=aE, f_err={"mae": np.nan, "rmse": np.nan},
             md5_test=None, interact_cut_off=None, use_E_cstr=True)
    path = tmp_path / "model.npz"
    np.savez_compressed(path, **m)
    for given in (path, str(path)):
        a = prd.load_model_arrays(given, energy_constraints=True)
        assert np.array_equal(a["alphas_E"], aE) and a["alphas_E"].dtype == np.float64
    with np.load(path, allow_pickle=False) as opened:
        a = prd.load_model_arrays(opened, energy_constraints=True)
        with pytest.raises(NotImplementedError):
            prd.load_model_arrays(opened)
    assert np.array_equal(a["alphas_E"], aE)
    np.testing.assert_array_equal(a["R_desc"], m["R_desc"].T)


@pytest.mark.parametrize("energy_constraints", [False, True])
def test_lattice_and_cut_off_refused_in_both_modes(golden_dir, energy_constraints):
    m = model_of(golden_dir)
    for extra in ({}, {"alphas_E": coefficients()}):
        for bad in ({"lattice": np.eye(3)}, {"interact_cut_off": 5.0}):
            if not energy_constraints and extra:
                continue                               # refused for alphas_E already
            with pytest.raises(NotImplementedError, match="lattice|cut-off"):
                prd.load_model_arrays(dict(m, **extra, **bad), energy_constraints=energy_constraints)


def test_abi_rejects_null_context():
    from sgdml_amd import _native

    lib = _native.load_library()
    assert lib.mlff_predict_set_energy_coefficients(None, None) == _native.MLFF_ERR_ARG


def test_docstrings_no_longer_claim_a_refusal():
    from sgdml_amd import model as mdl

    assert "refuses" not in mdl.__doc__
    assert "alphas_E" in prd.__doc__ and "alphas_E" in mdl.__doc__
