"""CPU: the masked mode's public surface — collate's true lengths, the model flag, the entry
points' ctypes rows (their agreement with the header is test_capi.py's)."""
import numpy as np
import pytest
import torch


def _items():
    rng = np.random.default_rng(0)
    items = []
    for n1, n2 in ((7, 5), (3, 9), (4, 1)):
        shape = lambda n: {"xyz": rng.normal(size=(n, 3)).astype(np.float32),  # noqa: E731
                           "mass": rng.random(n).astype(np.float32), "evals": rng.random(6).astype(np.float32),
                           "evecs": rng.normal(size=(n, 6)).astype(np.float32), "L": object()}
        items.append((shape(n1), shape(n2), {"obj_id": 1, "P": rng.integers(0, 3, size=(4, 2))}))
    return items


def test_collate_counts_returns_true_lengths():
    from dpfm_amd.dataset.helpers import collate, shape_to_device
    CAD, PC, _ = collate(_items(), counts=True)
    assert CAD["n"].dtype == torch.int32 and CAD["n"].tolist() == [7, 3, 4]
    assert PC["n"].dtype == torch.int32 and PC["n"].tolist() == [5, 9, 1]
    assert CAD["xyz"].shape == (3, 7, 3) and PC["xyz"].shape == (3, 9, 3)
    for part in (CAD, PC):  # the lengths are exactly the rows collate did not pad
        for b, n in enumerate(part["n"].tolist()):
            assert (part["xyz"][b, n:] == 0).all() and (part["xyz"][b, :n] != 0).any(1).all()
    moved = shape_to_device({"shape1": CAD, "shape2": PC}, torch.device("meta"))
    assert moved["shape1"]["n"].device.type == "meta" and moved["shape2"]["xyz"].device.type == "meta"


def test_collate_default_is_unchanged():
    from dpfm_amd.dataset.helpers import collate
    items = _items()
    CAD, PC, Obj = collate(items)
    CADc, PCc, Objc = collate(items, counts=True)
    assert list(CAD) == list(items[0][0]) and list(PC) == list(items[0][1])  # today's keys, in order
    assert "n" not in CAD and "n" not in PC
    assert [k for k in CADc if k != "n"] == list(CAD) and list(Obj) == list(Objc)
    for key in CAD:
        assert (CAD[key] is None and CADc[key] is None) or torch.equal(CAD[key], CADc[key])


def test_masked_model_state_dict_keys_unchanged():
    from dpfm_amd.models.dpfm import DPFMNet
    plain, masked = DPFMNet(), DPFMNet(masked=True)
    assert list(masked.state_dict().keys()) == list(plain.state_dict().keys())
    assert masked.masked and not plain.masked
    masked.load_state_dict(plain.state_dict(), strict=True)


def test_masked_forward_needs_lengths():
    from dpfm_amd.models.dpfm import DPFMNet
    shape = lambda n: {"xyz": torch.zeros(2, n, 3), "mass": torch.zeros(2, n), "evals": torch.zeros(2, 64),  # noqa: E731
                       "evecs": torch.zeros(2, n, 64)}
    model = DPFMNet(masked=True)
    with pytest.raises(ValueError, match='"n"'):
        model({"shape1": shape(8), "shape2": shape(6)})
    half = shape(8)
    half["n"] = torch.tensor([8, 3], dtype=torch.int32)
    with pytest.raises(ValueError, match='"n"'):
        model({"shape1": half, "shape2": shape(6)})


def test_new_entry_points_in_ctypes_table():
    from dpfm_amd import _lib
    P, I, I64, F = _lib._P, _lib._I, _lib._I64, _lib._F
    assert _lib.SIGNATURES["pk_attention_fwd_varlen"] == [P, P, P, I, I, I, I, I, I64, I64, P, P, P, P, P]
    assert _lib.SIGNATURES["pk_attention_bwd_varlen"] == [P, P, P, P, P, P, I, I, I, I, I, I64, I64, P, P, P, P, P, P,
                                                         I64, I64, P]
    assert _lib.SIGNATURES["pk_instnorm_relu_fwd_varlen"] == [P, I64, I, F, P, P, P, I, P, P]
    assert _lib.SIGNATURES["pk_instnorm_relu_bwd_varlen"] == [P, P, P, P, I64, I, P, I, P, P]
    assert _lib.SIGNATURES["pk_wbce_varlen"] == [P, P, I, P, P, I, I, P, P, P, P, P, P]
    # the existing entry points keep their positional signatures
    assert len(_lib.SIGNATURES["pk_attention_fwd"]) == 13 and len(_lib.SIGNATURES["pk_attention_bwd"]) == 20
    assert len(_lib.SIGNATURES["pk_instnorm_relu_fwd"]) == 8 and len(_lib.SIGNATURES["pk_wbce"]) == 11


def test_masked_keywords_exist_and_default_off():
    import inspect
    from dpfm_amd import attnprop, ops
    from dpfm_amd.modeling.dpfm import CrossAttentionRefinementNet
    from dpfm_amd.pipeline import InferStep, TrainStep, model_batch
    from dpfm_amd.utils.loss import DPFMLoss
    for fn, names in ((ops.attention, ("qlen", "klen")), (ops.instnorm_relu, ("lens",)),
                      (ops.weighted_bce_pair, ("n1", "n2")), (ops.dpfm_loss, ("n1", "n2")),
                      (attnprop.attn_prop_pair, ("nx", "nsrc")), (attnprop.attn_prop_residual, ("nx", "nsrc")),
                      (attnprop._prop_fwd, ("nx", "nsrc")), (attnprop._prop_bwd, ("nx", "nsrc")),
                      (DPFMLoss.forward_batched, ("n1", "n2")), (DPFMLoss.forward_batched_composed, ("n1", "n2")),
                      (CrossAttentionRefinementNet.forward, ("lengths",))):
        sig = inspect.signature(fn)
        for n in names:
            assert sig.parameters[n].default is None, (fn, n)
    for fn in (model_batch, TrainStep.__init__, InferStep.__init__):
        assert inspect.signature(fn).parameters["masked"].default is False
