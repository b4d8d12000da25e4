"""AvUC / EaU / EaC calibration losses without a GPU: the vectorised ATen chain against the reference's recorded outputs
(tests/golden/avuc.npz, tools/make_golden_avuc.py), gradcheck of the float64 chain, the numpy helpers, shapes, argument errors,
the alias, and the host side of the new C-ABI entry points."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import bayesian_torch_amd as bt
from bayesian_torch_amd.utils import _calibration as C
from bayesian_torch_amd.utils import avuc_loss as A
from bayesian_torch_amd.utils import uncertainty_calibration_loss as U

from avuc_cases import (AREA_NAMES, AVU_NAMES, EAU_NAMES, assert_avu_margin, assert_eau_margin, load, rel, rel_l2)

# both sides are f32 ATen on the same inputs and differ only in the order of the sums
REF_TOL = 1e-6
AUC_ABS_TOL = 2e-7


def _avu_module_run(mod, c, *extra):
    lg = torch.from_numpy(c["logits"]).clone().requires_grad_(True)
    loss = mod(lg, torch.from_numpy(c["labels"]), float(c["th"]), *extra)
    loss.sum().backward()
    return loss, lg.grad.numpy()


@pytest.mark.parametrize("name", AVU_NAMES)
def test_avuloss_matches_reference_avuc_loss(name):
    c = load()["avu"][name]
    assert_avu_margin(name, False)
    loss, grad = _avu_module_run(A.AvULoss(beta=float(c["beta"])), c)
    assert loss.shape == (1,) and loss.dtype == torch.float32
    print("%s: loss rel %.2e grad rel-L2 %.2e" % (name, rel(loss, c["ref1_loss"][0]), rel_l2(grad, c["ref1_dlogits"])))
    if float(c["ref1_loss"][0]) == 0.0:  # B = 1: AvU is exactly 1
        assert abs(float(loss)) <= 1e-7
    else:
        assert rel(loss, c["ref1_loss"][0]) <= REF_TOL
    if np.linalg.norm(c["ref1_dlogits"]) > 0:
        assert rel_l2(grad, c["ref1_dlogits"]) <= REF_TOL
    else:
        assert np.abs(grad).max() <= 1e-12


@pytest.mark.parametrize("name", AREA_NAMES)
def test_avuloss_matches_reference_uncertainty_calibration_loss(name):
    c = load()["avu"][name]
    loss, grad = _avu_module_run(U.AvULoss(beta=float(c["beta"])), c)
    assert loss.shape == () and loss.dtype == torch.float32
    ref_grad = c["ref1_dlogits"] + c["ref2_dlogits_minus_ref1"]
    print("%s: loss rel %.2e grad rel-L2 %.2e" % (name, rel(loss, c["ref2_loss"][0]), rel_l2(grad, ref_grad)))
    assert rel(loss, c["ref2_loss"][0]) <= REF_TOL
    assert rel_l2(grad, ref_grad) <= REF_TOL


@pytest.mark.parametrize("name", AREA_NAMES)
def test_auavuloss_value_matches_reference_auc_avu(name):
    c = load()["avu"][name]
    assert_avu_margin(name, True)
    lg = torch.from_numpy(c["logits"]).clone().requires_grad_(True)
    loss, auc = A.AUAvULoss(beta=float(c["beta"]))(lg, torch.from_numpy(c["labels"]))
    assert loss.shape == (1,) and auc.shape == (1,)
    assert loss.requires_grad and auc.requires_grad
    print("%s: auc %.8f reference %.8f" % (name, float(auc), float(c["ref_auc"])))
    assert abs(float(auc) - float(c["ref_auc"])) <= AUC_ABS_TOL
    assert rel(loss, -float(c["beta"]) * np.log(float(c["ref_auc"]) + 1e-10)) <= REF_TOL
    (loss + auc).sum().backward()
    assert np.isfinite(lg.grad.numpy()).all() and np.abs(lg.grad.numpy()).max() > 0


@pytest.mark.parametrize("name", EAU_NAMES)
@pytest.mark.parametrize("form", ["eau", "eac"])
def test_eau_eac_match_reference(name, form):
    c = load()["eau"][name]
    assert_eau_margin(name)
    e = torch.from_numpy(c["error"]).clone().requires_grad_(True)
    if form == "eau":
        o = torch.from_numpy(c["unc"]).clone().requires_grad_(True)
        loss = U.EaULoss(beta=float(c["beta"]))(e, o, float(c["error_th"]), float(c["unc_th"]))
    else:
        o = torch.from_numpy(c["conf"]).clone().requires_grad_(True)
        loss = U.EaCLoss(beta=float(c["beta"]))(e, o, float(c["error_th"]), float(c["conf_th"]))
    assert loss.shape == ()
    loss.backward()
    assert rel(loss, c[form + "_loss"][0]) <= REF_TOL
    assert rel_l2(e.grad.numpy(), c[form + "_derror"]) <= REF_TOL
    assert rel_l2(o.grad.numpy(), c[form + "_dother"]) <= REF_TOL


def test_gradcheck_of_the_float64_chain_for_all_five_losses():
    """the margins of the (7, 10) case keep every membership fixed under gradcheck's 1e-6 steps: the loss is locally smooth"""
    c = load()["avu"]["b7_c10"]
    labels = torch.from_numpy(c["labels"])
    lg = torch.from_numpy(c["logits"]).double().requires_grad_(True)
    th, beta = float(c["th"]), 2.0
    assert torch.autograd.gradcheck(lambda z: A.AvULoss(beta)(z, labels, th), (lg,))
    assert torch.autograd.gradcheck(lambda z: U.AvULoss(beta)(z, labels, th), (lg,))
    assert torch.autograd.gradcheck(lambda z: A.AUAvULoss(beta)(z, labels), (lg,))
    e = load()["eau"]["e7"]
    err = torch.from_numpy(e["error"]).double().requires_grad_(True)
    unc = torch.from_numpy(e["unc"]).double().requires_grad_(True)
    conf = torch.from_numpy(e["conf"]).double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: U.EaULoss(beta)(a, b, float(e["error_th"]), float(e["unc_th"])), (err, unc))
    assert torch.autograd.gradcheck(lambda a, b: U.EaCLoss(beta)(a, b, float(e["error_th"]), float(e["conf_th"])), (err, conf))


def test_numpy_helpers_match_reference_outputs():
    n = load()["np"]
    mc = n["mc_preds"]
    np.testing.assert_allclose(A.entropy(mc), n["entropy"], rtol=1e-12)
    np.testing.assert_allclose(A.predictive_entropy(mc), n["predictive_entropy"], rtol=1e-12)
    np.testing.assert_allclose(A.mutual_information(mc), n["mutual_information"], rtol=1e-10, atol=1e-15)
    avu, ths = A.eval_avu(n["pred"], n["true"], n["predictive_entropy"])
    assert avu.shape == (21,) and ths.shape == (21,)
    np.testing.assert_allclose(avu, n["eval_avu"], rtol=1e-12)
    np.testing.assert_allclose(ths, n["eval_avu_th"], rtol=1e-15)
    got = A.accuracy_vs_uncertainty(n["pred"], n["true"], n["predictive_entropy"], float(n["th"]))
    assert abs(got - float(n["accuracy_vs_uncertainty"])) <= 1e-15


def test_type_1_and_stacked_logits_raise_value_error():
    c = load()["avu"]["b7_c10"]
    lg, lb = torch.from_numpy(c["logits"]), torch.from_numpy(c["labels"])
    with pytest.raises(ValueError, match="type=1"):
        A.AvULoss()(lg, lb, 0.5, type=1)
    with pytest.raises(ValueError, match="type=1"):
        A.AUAvULoss()(lg, lb, type=1)
    with pytest.raises(ValueError, match="batch, classes"):
        A.AvULoss()(lg.unsqueeze(0), lb, 0.5)


def test_column_vectors_equal_flattened_inputs():
    e = load()["eau"]["e7"]
    err, unc, conf = (torch.from_numpy(e[k]) for k in ("error", "unc", "conf"))
    et, ut, ct = float(e["error_th"]), float(e["unc_th"]), float(e["conf_th"])
    flat = U.EaULoss()(err, unc, et, ut)
    assert torch.equal(U.EaULoss()(err[:, None], unc[:, None], et, ut), flat)
    assert float(flat) < 20.0  # not the reference's degenerate -log(1e-10) = 23.03
    assert torch.equal(U.EaCLoss()(err[:, None], conf[:, None], et, ct), U.EaCLoss()(err, conf, et, ct))


def test_tensor_threshold_equals_python_threshold_on_cpu():
    c = load()["avu"]["b7_c10"]
    lg, lb = torch.from_numpy(c["logits"]), torch.from_numpy(c["labels"])
    assert torch.equal(A.AvULoss()(lg, lb, torch.tensor(float(c["th"]))), A.AvULoss()(lg, lb, float(c["th"])))


def test_install_alias_resolves_both_modules():
    bt.install_alias()
    assert importlib.import_module("bayesian_torch.utils.avuc_loss") is A
    assert importlib.import_module("bayesian_torch.utils.uncertainty_calibration_loss") is U
    from bayesian_torch.utils.avuc_loss import AvULoss, AUAvULoss  # noqa: F401
    from bayesian_torch.utils.uncertainty_calibration_loss import EaULoss, EaCLoss  # noqa: F401


def test_cabi_calibration_entry_points_without_gpu():
    """host-side argument validation: every call returns before anything is launched"""
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    assert L.btx_abi_version() == 9  # additive: the ABI number does not move
    for n in ("btx_calib_workspace_bytes", "btx_avu_fwd", "btx_avu_bwd", "btx_eau_fwd", "btx_eau_bwd"):
        assert n in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.lib_path()), n)
    sizes = [L.btx_calib_workspace_bytes(b) for b in (0, 1, 7, 64, 1500, 100000)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    one = ctypes.c_void_p(256)
    big = sizes[-1]
    assert L.btx_avu_fwd(None, one, 4, 10, 0, 0, 0.5, None, 1.0, one, one, big, None) == -1
    assert L.btx_avu_fwd(one, None, 4, 10, 0, 0, 0.5, None, 1.0, one, one, big, None) == -1
    assert L.btx_avu_fwd(one, one, 4, 10, 0, 0, 0.5, None, 1.0, None, one, big, None) == -1
    assert L.btx_avu_fwd(one, one, 4, 10, 0, 0, 0.5, None, 1.0, one, None, big, None) == -1
    assert L.btx_avu_fwd(one, one, 0, 10, 0, 0, 0.5, None, 1.0, one, one, big, None) == -2
    assert L.btx_avu_fwd(one, one, 4, 0, 0, 0, 0.5, None, 1.0, one, one, big, None) == -2
    assert L.btx_avu_fwd(one, one, 4, 10, 0, 2, 0.5, None, 1.0, one, one, big, None) == -2
    assert L.btx_avu_fwd(one, one, 4, 10, 7, 0, 0.5, None, 1.0, one, one, big, None) == -5
    assert L.btx_avu_fwd(one, one, 4, 10, 0, 0, 0.5, None, 1.0, one, one, 16, None) == -4
    assert L.btx_avu_bwd(None, 4, 10, 0, one, None, one, big, one, None) == -1
    assert L.btx_avu_bwd(one, 4, 10, 0, None, None, one, big, one, None) == -1
    assert L.btx_avu_bwd(one, 4, -1, 0, one, None, one, big, one, None) == -2
    assert L.btx_avu_bwd(one, 4, 10, 0, one, None, one, 16, one, None) == -4
    assert L.btx_eau_fwd(None, one, 4, 0, 0.5, None, 0.5, None, 1.0, one, one, big, None) == -1
    assert L.btx_eau_fwd(one, one, 0, 0, 0.5, None, 0.5, None, 1.0, one, one, big, None) == -2
    assert L.btx_eau_fwd(one, one, 4, 3, 0.5, None, 0.5, None, 1.0, one, one, big, None) == -2
    assert L.btx_eau_bwd(one, one, 4, 0, None, one, big, one, one, None) == -1
    assert L.btx_eau_bwd(one, one, 4, 0, one, one, big, None, None, None) == -1
    assert L.btx_eau_bwd(one, one, -3, 1, one, one, big, one, one, None) == -2
