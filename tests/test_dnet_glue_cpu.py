"""CPU: the pure pieces of DNET's launch orchestration (dnet.py): the layer classifier the three
prologues share, the s[o] views of one buffer, the exactly-2x predicate and DNETFn's argument bundle."""
import itertools
import types

import pytest
import torch


@pytest.fixture(scope="module")
def D(nconv_amd):
    return nconv_amd.dnet


def _fake_weight(cuda=True, dtype=torch.float32, contiguous=True):
    return types.SimpleNamespace(is_cuda=cuda, dtype=dtype, is_contiguous=lambda: contiguous)


def test_layer_class_hooks(nconv_amd, D):
    N = nconv_amd.nconv
    assert D._layer_class(N.NConv2d(1, 8, (5, 5), pos_fn=None))[0] == "none"
    ours = N.NConv2d(1, 8, (5, 5))
    assert D._layer_class(ours)[0] == "ours"
    ours.register_forward_pre_hook(lambda mod, inputs: None)  # ours plus a second one: run as hooks
    assert D._layer_class(ours)[0] == "foreign"
    for pos_fn in ("exp", "softmax", "sigmoid"):
        assert D._layer_class(N.NConv2d(1, 8, (5, 5), pos_fn=pos_fn))[0] == "foreign"
    other = N.NConv2d(1, 8, (5, 5), pos_fn=None)
    N.EnforcePos.apply(other, "bias", "softplus")  # our hook class on another parameter
    assert D._layer_class(other)[0] == "foreign"


def test_layer_class_weight(nconv_amd, D):
    m = nconv_amd.nconv.NConv2d(8, 8, (5, 5))
    assert D._layer_class(m) == ("ours", False)  # a CPU weight
    fake = lambda **kw: types.SimpleNamespace(_forward_pre_hooks={}, weight=_fake_weight(**kw))  # noqa: E731
    assert D._layer_class(fake()) == ("none", True)
    assert D._layer_class(fake(cuda=False)) == ("none", False)
    assert D._layer_class(fake(contiguous=False)) == ("none", False)
    assert D._layer_class(fake(dtype=torch.float16)) == ("none", False)
    m.weight.data = m.weight.data.transpose(2, 3).contiguous().transpose(2, 3)  # non-contiguous, on the CPU
    assert not m.weight.is_contiguous() and D._layer_class(m)[1] is False


def test_wsum_views_of_the_nine_layers(nconv_amd, D):
    net = nconv_amd.DNET(32)
    weights = [getattr(net, n).weight.data for n in D.LAYERS]
    views = D._wsum_views(weights, torch.device("cpu"))
    assert [v.numel() for v in views] == [8] * 8 + [1]
    assert [v.storage_offset() for v in views] == [8 * k for k in range(9)]
    base = views[0].untyped_storage().data_ptr()
    assert all(v.untyped_storage().data_ptr() == base and v.is_contiguous() and v.dtype == torch.float32
               for v in views)
    assert views[0].untyped_storage().nbytes() == 65 * 4


def test_exact_up(D):
    assert D._exact_up(64, 96) and D._exact_up(16, 16)
    assert not D._exact_up(63, 96) and not D._exact_up(64, 97) and not D._exact_up(63, 97)


@pytest.mark.parametrize("absent", list(itertools.product((False, True), repeat=3)))
def test_dnet_args_round_trip(D, absent):
    layers = tuple(tuple(torch.full((1,), 3.0 * i + j) for j in range(3)) for i in range(9))
    wph, w21, wbox = (None if a else torch.zeros(k + 1) for k, a in enumerate(absent))
    flat = D.DNETArgs(layers, wph, w21, wbox).flatten()
    assert len(flat) == 30  # fixed arity: what DNETFn.backward returns gradients for
    assert [float(t) for t in flat[:27]] == [float(k) for k in range(27)]
    back = D.DNETArgs.unflatten(flat)
    assert all(a is b for x, y in zip(back.layers, layers) for a, b in zip(x, y)) and len(back.layers) == 9
    assert back.wph is wph and back.w21 is w21 and back.wbox is wbox


ACT_ORDER = ("x1 c1 x2 c2 x3 c3 x4 c4 x5 c5 x6 c6 x7 c7 x8 c8 x9 c9 "
             "p2x p2c a2 p3x p3c a3 p4x p4c a4").split()


@pytest.mark.parametrize("pooled", [True, False])
def test_train_acts_round_trip(D, pooled):
    """DNETFn's saved activations: the flat order handed to save_for_backward is the record's field order, 27
    tensors with the pooled graph's copies and argmax codes and the first 18 without; the backward rebuilds the
    record from that flat form."""
    assert list(D.TrainActs._fields) == ACT_ORDER
    n = 27 if pooled else 18
    named = {name: torch.full((1,), float(k)) for k, name in enumerate(ACT_ORDER[:n])}
    acts = D.TrainActs(**named)
    flat = acts.flatten()
    assert len(flat) == n and all(t is named[name] for t, name in zip(flat, ACT_ORDER))
    back = D.TrainActs(*flat)
    assert back == acts and all(getattr(back, name) is named.get(name) for name in ACT_ORDER)
    assert all(x is named[f"x{k}"] and c is named[f"c{k}"] for k, (x, c) in enumerate(back.outputs(), 1))
    assert len(back.outputs()) == 9
