"""CPU: the weight-gradient seam (dpfm_amd/wgrad.py). Recording a layer's (x, dy) products for
the grouped launch touches no device, so the routing every fused node's backward goes through is
checked here on CPU tensors; what the grouped launch computes is tests/test_pipeline_gpu.py's."""
import pytest
import torch
import torch.nn as nn


def test_weight_grad_records_for_the_active_recorder_only():
    from dpfm_amd import wgrad
    from dpfm_amd._lib import PoseKernError
    O, I, R = 6, 1, 5
    weight = nn.Parameter(torch.randn(O, I, 1))  # a Conv1d(k=1) weight: recorded as [O, I]
    bias = nn.Parameter(torch.randn(O))
    time = nn.Parameter(torch.rand(4))           # a parameter one kernel writes whole (direct)
    side = wgrad.GroupedWgrad([weight, bias], direct_params=[time])
    x0, dy0, x1, dy1 = torch.randn(R, I), torch.randn(R, O), torch.randn(R, I), torch.randn(R, O)
    acc = (object(), object())

    side.begin()
    try:
        assert weight.grad is side.bufs[id(weight)] and bias.grad is side.bufs[id(bias)]
        assert wgrad.weight_grad(x0, dy0, weight, bias, False) == (None, None)
        assert wgrad.weight_grad(x1, dy1, weight, bias, False, acc=acc) is acc  # untouched
        assert len(side.calls) == 2
        assert [c[5] for c in side.calls] == [False, True]  # the accumulate flags
        for (x, dy, cf, dw, db, _), (ex, edy) in zip(side.calls, ((x0, dy0), (x1, dy1))):
            assert x is ex and dy is edy and cf is False
            assert dw.shape == (O, I) and dw.data_ptr() == weight.grad.data_ptr()
            assert db is bias.grad
        assert wgrad.direct_grad(time) is time.grad is side.bufs[id(time)]
        assert wgrad.direct_grad(time) is None       # handed out once per backward
        assert wgrad.direct_grad(nn.Parameter(torch.zeros(4))) is None  # not the recorder's
    finally:
        side.end(run=False)

    assert side.calls == [] and wgrad.direct_grad(time) is None
    with pytest.raises(PoseKernError):  # no recorder: the launch itself, and there is no CPU fallback
        wgrad.weight_grad(x0, dy0, weight, bias, False)
    assert side.calls == []


def test_weight_grad_computes_for_a_layer_the_recorder_does_not_own():
    from dpfm_amd import layers, wgrad
    from dpfm_amd._lib import PoseKernError
    assert layers.GroupedWgrad is wgrad.GroupedWgrad
    weight, bias = nn.Parameter(torch.randn(3, 2)), nn.Parameter(torch.randn(3))
    other = nn.Parameter(torch.randn(3, 2))
    side = wgrad.GroupedWgrad([weight])  # the bias is not the recorder's: neither is the layer
    side.begin()
    try:
        for w, b in ((other, None), (weight, bias)):
            with pytest.raises(PoseKernError):
                wgrad.weight_grad(torch.randn(4, 2), torch.randn(4, 3), w, b, False)
        assert side.calls == []
        assert wgrad.weight_grad(torch.randn(4, 2), torch.randn(4, 3), weight, None, False) == (None, None)
        assert len(side.calls) == 1 and side.calls[0][4] is None
    finally:
        side.end(run=False)
