"""CPU: nconv.bwd_io, the host step of layer_backward that turns the backward's records (InputGrads, PoolGrad,
HeadBwd, TailBwd) into an nconv_bwd_io and the head / tail descriptors, and the rule choosing the entry point.
bwd_io reads data_ptr() and shapes only, so CPU tensors and made-up workspace addresses serve."""
import ctypes
import itertools

import pytest
import torch

HEAD_WS, TAIL_WS = (0x7000_0000, 4096), (0x7100_0000, 512)
FEATURES = ("pool", "head", "crop", "gcout")


@pytest.fixture(scope="module")
def N(nconv_amd):
    return nconv_amd.nconv


@pytest.fixture(scope="module")
def case(nconv_amd, N):
    """nconv6 at 8 x 12 (UPCAT, 3x3, no padding: a 6 x 10 grid) with DNET's nconv1 as its head and nconv7 as its
    tail, nconv7's planes a 7 x 11 window of its 10 x 14 grid. Every tensor is its own allocation."""
    lib = nconv_amd._lib
    t = lambda *s: torch.zeros(*s)  # noqa: E731
    k = dict(spec=N.LayerSpec(16, 8, (3, 3), mode=lib.UPCAT_UP_FIRST),
             ops=N.Operands(t(2, 8, 8, 12), t(2, 8, 8, 12), t(2, 8, 4, 6), t(2, 8, 4, 6), t(8, 16, 3, 3), t(8), t(8)),
             y=t(2, 8, 6, 10), co=t(2, 8, 6, 10), gy=t(2, 8, 6, 10), gco=t(2, 8, 6, 10),
             gin=N.InputGrads(t(2, 8, 8, 12), t(2, 8, 8, 12), t(2, 8, 4, 6), t(2, 8, 4, 6)), gw=t(8, 16, 3, 3), gb=t(8),
             box=t(1024), pool=N.PoolGrad(t(2, 8, 3, 5), t(2, 8, 3, 5), torch.zeros(2, 8, 3, 5, dtype=torch.int32)),
             head=N.HeadBwd(N.LayerSpec(1, 8, (5, 5), padding=(2, 2), mode=lib.THRESH), t(2, 1, 8, 12), t(8, 1, 5, 5),
                            t(8), t(8), t(8, 1, 5, 5), t(8)),
             tail=N.TailBwd(N.LayerSpec(8, 1, (1, 1), padding=(2, 2)), t(1, 8, 1, 1), t(1), t(1), t(2, 1, 7, 11),
                            t(2, 1, 7, 11), t(2, 1, 7, 11), t(1, 8, 1, 1)),
             tail_gcout=t(2, 1, 7, 11))
    return k


def _records(k, features):
    """(pool_grad, head, tail) of a call with these features; the tail without a crop holds the same planes."""
    tail = None
    if "crop" in features or "gcout" in features:
        tail = k["tail"]._replace(crop0=1 if "crop" in features else None,
                                  gcout=k["tail_gcout"] if "gcout" in features else None)
    return (k["pool"] if "pool" in features else None), (k["head"] if "head" in features else None), tail


def _build(N, k, pool, head, tail, gin=None):
    tailed = tail is not None  # (a tail's caller passes no gy / gco of the layer itself)
    return N.bwd_io(k["y"], k["co"], None if tailed else k["gy"], None if tailed else k["gco"],
                    k["gin"] if gin is None else gin, k["gw"], k["gb"], pool, head, tail, k["box"],
                    HEAD_WS if head is not None else (None, 0), TAIL_WS if tail is not None else (None, 0))


def _fields(lib, io):
    """Every field of an nconv_bwd_io by name: pointers as addresses (None: null), the head / tail descriptors
    as their bytes."""
    out = {}
    for name, typ in lib.NconvBwdIo._fields_:
        v = getattr(io, name)
        if typ is ctypes.POINTER(lib.NconvLayer):
            v = bytes(v.contents) if v else None
        out[name] = v
    return out


def _expected(lib, k, pool, head, tail):
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    gin = k["gin"]
    want = {name: (0 if typ in (ctypes.c_int, ctypes.c_size_t) else None) for name, typ in lib.NconvBwdIo._fields_}
    want.update(y=p(k["y"]), cout=p(k["co"]), gxa=p(gin.gxa), gca=p(gin.gca), gxb=p(gin.gxb), gcb=p(gin.gcb),
                gw=p(k["gw"]), gbias=p(k["gb"]), box_weights=p(k["box"]))
    if tail is None:
        want.update(gy=p(k["gy"]), gcout=p(k["gco"]))
    if pool is not None:
        want.update(gy_pool=p(pool.gy), gcout_pool=p(pool.gcout), pool_argmax=p(pool.argmax))
    if head is not None:
        HL = head.spec.descriptor(head.S, None, None, None, head.weight, head.bias, head.wsum)
        want.update(head=bytes(HL), head_workspace=HEAD_WS[0], head_workspace_bytes=HEAD_WS[1], head_gw=p(head.gw),
                    head_gbias=p(head.gb))
    if tail is not None:
        TL = tail.spec.descriptor(k["y"], k["co"], None, None, tail.weight, tail.bias, tail.wsum)
        want.update(tail=bytes(TL), tail_y=p(tail.y), tail_cout=p(tail.cout), tail_gy=p(tail.gy), tail_gw=p(tail.gw),
                    tail_workspace=TAIL_WS[0], tail_workspace_bytes=TAIL_WS[1])
        if tail.crop0 is not None:
            want.update(tail_crop0=1, tail_h=tail.y.shape[2], tail_w=tail.y.shape[3])
    return want


@pytest.mark.parametrize("features", [(), *[(f,) for f in FEATURES], FEATURES], ids=lambda f: "+".join(f) or "plain")
def test_bwd_io_fields(nconv_amd, N, case, features):
    """Every field of nconv_bwd_io is the data_ptr() of the tensor its record names, null (0 for the integers)
    where the record holds None or is absent; the head / tail descriptors are LayerSpec.descriptor's for
    (S, None, None, None) and (y, co, None, None); tail_crop0 / tail_h / tail_w are (1, y's rows, y's columns)
    with a crop and (0, 0, 0) without."""
    lib = nconv_amd._lib
    pool, head, tail = _records(case, features)
    io, HL, TL = _build(N, case, pool, head, tail)
    got, want = _fields(lib, io), _expected(lib, case, pool, head, tail)
    assert set(got) == set(want)
    for name in want:
        assert got[name] == want[name], name
    assert (got["tail_crop0"], got["tail_h"], got["tail_w"]) == ((1, 7, 11) if "crop" in features else (0, 0, 0))
    assert (HL is None) == (head is None) and (TL is None) == (tail is None)
    if head is not None:  # io points at the returned descriptors themselves
        assert ctypes.addressof(io.head.contents) == ctypes.addressof(HL)
        assert (HL.B, HL.Cin, HL.H, HL.W, HL.Cout, HL.Ho, HL.Wo, HL.KH, HL.PH) == (2, 1, 8, 12, 8, 8, 12, 5, 2)
        assert (HL.a.x, HL.a.c, HL.b.x) == (head.S.data_ptr(), None, None)
    if tail is not None:
        assert ctypes.addressof(io.tail.contents) == ctypes.addressof(TL)
        assert (TL.B, TL.Cin, TL.H, TL.W, TL.Cout, TL.Ho, TL.Wo, TL.KH, TL.PH) == (2, 8, 6, 10, 1, 10, 14, 1, 2)
        assert (TL.a.x, TL.a.c, TL.b.x) == (case["y"].data_ptr(), case["co"].data_ptr(), None)


def test_bwd_io_skipped_input_gradients(nconv_amd, N, case):
    """InputGrads() names no destination: the weight-gradient half of the side-stream split."""
    assert N.InputGrads() == (None, None, None, None)
    got = _fields(nconv_amd._lib, _build(N, case, None, None, None, gin=N.InputGrads())[0])
    assert (got["gxa"], got["gca"], got["gxb"], got["gcb"]) == (None, None, None, None)
    assert got["gw"] == case["gw"].data_ptr() and got["gbias"] == case["gb"].data_ptr()


@pytest.mark.parametrize("features", [("crop",), ("gcout",), FEATURES], ids="+".join)
def test_tail_without_gw_changes_tail_gw_only(nconv_amd, N, case, features):
    """The input-gradient half of the side-stream split: tail._replace(gw=None) leaves every field but tail_gw."""
    lib = nconv_amd._lib
    pool, head, tail = _records(case, features)
    less = tail._replace(gw=None)
    assert less.gw is None and all(a is b for f, a, b in zip(tail._fields, tail, less) if f != "gw")
    assert N.tail_conf_entry(less) == N.tail_conf_entry(tail)
    full, half = (_fields(lib, _build(N, case, pool, head, t)[0]) for t in (tail, less))
    assert full["tail_gw"] == tail.gw.data_ptr() and half["tail_gw"] is None
    assert {k: v for k, v in full.items() if k != "tail_gw"} == {k: v for k, v in half.items() if k != "tail_gw"}


@pytest.mark.parametrize("conf_entry,gcout,entry", [
    (False, False, "nconv_bwd_ex"), (True, False, "nconv_bwd_tail_conf"), (False, True, "nconv_bwd_tail_conf"),
    (True, True, "nconv_bwd_tail_conf")])
def test_tail_entry_point_rule(N, case, conf_entry, gcout, entry):
    tail = case["tail"]._replace(gcout=case["tail_gcout"] if gcout else None, conf_entry=conf_entry)
    assert N.tail_conf_entry(tail) is (entry == "nconv_bwd_tail_conf")
    for crop0 in (None, 1):  # the crop origin has no say
        assert N.tail_conf_entry(tail._replace(crop0=crop0)) is (entry == "nconv_bwd_tail_conf")


def test_no_tail_is_nconv_bwd_ex(N, case):
    assert N.tail_conf_entry(None) is False
    assert (case["tail"].crop0, case["tail"].gcout, case["tail"].conf_entry) == (None, None, False)  # the defaults


def test_records_unpack_in_field_order(N, case):
    """The records are tuples in the order of their fields: Operands is LayerSpec.descriptor's argument list."""
    assert N.Operands._fields == ("xa", "ca", "xb", "cb", "weight", "bias", "wsum")
    assert N.InputGrads._fields == ("gxa", "gca", "gxb", "gcb")
    assert N.PoolGrad._fields == ("gy", "gcout", "argmax")
    assert N.HeadBwd._fields == ("spec", "S", "weight", "bias", "wsum", "gw", "gb")
    assert N.TailBwd._fields == ("spec", "weight", "bias", "wsum", "y", "cout", "gy", "gw", "crop0", "gcout",
                                 "conf_entry")
    ops = case["ops"]
    L = case["spec"].descriptor(*ops)
    assert (L.a.x, L.a.c, L.b.x, L.b.c) == tuple(t.data_ptr() for t in itertools.islice(ops, 4))
    assert (L.weight, L.bias, L.wsum) == (ops.weight.data_ptr(), ops.bias.data_ptr(), ops.wsum.data_ptr())
    assert (L.H, L.W, L.Ho, L.Wo) == (8, 12, 6, 10)
