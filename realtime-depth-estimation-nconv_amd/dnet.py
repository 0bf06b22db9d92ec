"""DNET / SETP1_NCONV — drop-in for the reference's unguided NConv U-Net (models/step1.py:15-94).

The 9-layer graph (step1.py:51-94) runs as one libnconv launch per layer with the glue fused
into each layer's load stage:

    nconv1   THRESH      c0 = (S > 0.01), x0 = S                     step1.py:53-56
    nconv2   PLAIN                                                  step1.py:57
    down1-3  POOL2       independent 2x2 max-pool of x and c         step1.py:62-75
    nconv4/5 UPCAT_SKIP  cat(skip, nearest-up(low))                  step1.py:78-85
    nconv6   UPCAT_UP    cat(nearest-up(low), skip), padding 0       step1.py:88-90
    nconv7   PLAIN       1x1, default padding 2                      step1.py:92
    crop     [1:481, 1:641] (literal, default) or [1:H+1, 1:W+1]     step1.py:94

Without autograd (inference) nconv6 and nconv7 are fused into one launch that writes the cropped
output directly. EnforcePos pre-hooks of all nine layers are applied in one launch in training
mode, before any layer runs (the reference applies each right before its layer; the layers share
no weights, so the results are identical).
"""
import dataclasses
import itertools
import math
import os
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib, _streams, export, nconv
from .nconv import (EnforcePos, HeadBwd, InputGrads, NConv2d, Operands, PoolGrad, TailBwd, WgradReduce,
                    _require_device, head_weights, layer_backward, layer_forward_head, layer_forward_pooled,
                    layer_forward_raw, nconv_layer, phase_weights, train_prologue, weight_prep)

LAYERS = ("nconv1", "nconv2", "nconv_down1", "nconv_down2", "nconv_down3", "nconv4", "nconv5",
          "nconv6", "nconv7")


# Training forward in batch slices on this many streams (DNETFn.forward): the exact-fp32 pooled
# graph with the fused head and tail only; 1 = one launch per layer over the whole batch
TRAIN_FWD_STREAMS = int(os.environ.get("NCONV_TRAIN_FWD_STREAMS", "2"))

# Exact-fp32 training (DNETFn, pooled graph): the forward's head fused; nconv7's backward inside
# nconv6's and nconv1's weight gradient inside nconv2's input gradient (nconv_bwd_ex tail / head);
# the weight gradients on a second stream, concurrent with the input-gradient chain. Switches for
# tests.
FUSE_TAIL_BWD = True
FUSE_HEAD_BWD = True
FUSE_HEAD_FWD = True  # the training forward's nconv1 + nconv2 as the exact fused head (nconv_fwd_head)
FUSE_TAIL_FWD = True  # ... and nconv6 + nconv7 as the fused tail (nconv_fwd_tail over nconv7's whole grid)

# The training backward's weight gradients on one side stream (two round-robin streams measured
# slower: 2.20 -> 2.26 ms per graphed step, profiles/r5_ab_two_wgrad_streams.log), except the last
# layer's (nconv2's, WGRAD_LAST_MAIN): it runs on the main stream after that layer's input
# gradient, which is the main stream's last kernel, instead of queueing behind the side stream's
# backlog while the main stream idles
WGRAD_STREAM = True
WGRAD_LAST_MAIN = True


def _exact_up(H, W):
    """nconv6's skip input (nconv2's grid: the input's, H x W) is exactly twice nconv5's grid (the
    pooled one, H // 2 x W // 2): the phase form of nconv6, the fused tails, the cropped output."""
    return H % 2 == 0 and W % 2 == 0


def _layer_class(m):
    """(hooks, usable) of one NConv2d: its forward pre-hooks are "none", "ours" (exactly this
    package's softplus EnforcePos on the weight, which the prologue kernels apply themselves) or
    "foreign" (anything else: run as hooks); usable: the weight is a contiguous fp32 device tensor."""
    hooks, w = list(m._forward_pre_hooks.values()), m.weight
    ours = len(hooks) == 1 and isinstance(hooks[0], EnforcePos) and hooks[0].name == "weight" \
        and hooks[0].pos_fn.lower() == "softplus"
    kind = "none" if not hooks else "ours" if ours else "foreign"
    return kind, w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()


def _wsum_views(weights, device):
    """One s[o] vector per layer (weight.shape[0] elements), consecutive views of one buffer."""
    buf = torch.empty(sum(w.shape[0] for w in weights), device=device, dtype=torch.float32)
    return list(buf.split([w.shape[0] for w in weights]))


class DNETArgs(NamedTuple):
    """DNETFn's tensor arguments after S: layers = the nine (weight, bias, s[o]) in LAYERS order;
    wph = the phase weights of nconv4/5/6 (a (3, 1024) tensor, DNET._phase_weights) or None; w21 =
    the exact head's weights (None: built by the forward); wbox = the box weights of nconv4/5/6 (a
    (3, 1024) tensor; None: built by the backward), the last two from DNET._train_prologue."""
    layers: tuple
    wph: Optional[torch.Tensor] = None
    w21: Optional[torch.Tensor] = None
    wbox: Optional[torch.Tensor] = None

    def flatten(self):  # the fixed-arity form autograd sees (absent entries stay None)
        return (*itertools.chain.from_iterable(self.layers), self.wph, self.w21, self.wbox)

    @classmethod
    def unflatten(cls, p):
        return cls(tuple(tuple(p[3 * i:3 * i + 3]) for i in range(9)), *p[27:])


def _batch_rows(full, B, b0, b1):
    """The output allocator (nconv._outputs) of one batch slice's launches in the sliced training
    forward: the i-th output of the slice's launches = rows b0:b1 of the full-batch tensor full[i],
    which the first slice to ask for it allocates."""
    it = itertools.count()

    def rows(shapes, dtypes, device):
        out = []
        for sh, dt in zip(shapes, dtypes):
            i = next(it)
            if i == len(full):
                full.append(torch.empty((B,) + tuple(sh[1:]), device=device, dtype=dt))
            out.append(full[i][b0:b1])
        return out
    return rows


class TrainActs(NamedTuple):
    """What DNETFn's forward keeps for its backward, in the order it is saved: the nine layers'
    outputs (x, c) in LAYERS order, then (pooled graph only) the 2x2-pooled copies of nconv2's,
    down1's and down2's outputs (p2, p3, p4) with their pooling argmax codes (a2, a3, a4)."""
    x1: torch.Tensor
    c1: torch.Tensor
    x2: torch.Tensor
    c2: torch.Tensor
    x3: torch.Tensor
    c3: torch.Tensor
    x4: torch.Tensor
    c4: torch.Tensor
    x5: torch.Tensor
    c5: torch.Tensor
    x6: torch.Tensor
    c6: torch.Tensor
    x7: torch.Tensor
    c7: torch.Tensor
    x8: torch.Tensor
    c8: torch.Tensor
    x9: torch.Tensor
    c9: torch.Tensor
    p2x: Optional[torch.Tensor] = None
    p2c: Optional[torch.Tensor] = None
    a2: Optional[torch.Tensor] = None
    p3x: Optional[torch.Tensor] = None
    p3c: Optional[torch.Tensor] = None
    a3: Optional[torch.Tensor] = None
    p4x: Optional[torch.Tensor] = None
    p4c: Optional[torch.Tensor] = None
    a4: Optional[torch.Tensor] = None

    def flatten(self):  # 18 tensors, or 27 with the pooled graph's: what save_for_backward takes
        return tuple(self) if self.p2x is not None else tuple(self)[:18]

    def outputs(self):  # the nine layers' (x, c)
        return tuple(zip(self[0:18:2], self[1:18:2]))


class _BwdLayer(NamedTuple):
    """One layer in DNETFn.backward: its spec and (weight, bias, s[o]), and where its weight and
    bias gradients go (None: not needed)."""
    spec: nconv.LayerSpec
    weight: torch.Tensor
    bias: torch.Tensor
    wsum: torch.Tensor
    gw: Optional[torch.Tensor]
    gb: Optional[torch.Tensor]

    def operands(self, a, b=(None, None)):  # a, b: the (x, c) pairs the layer reads
        return Operands(*a, *b, self.weight, self.bias, self.wsum)


def _train_fwd_chain(sp, W, S, w21, wph, crop, out, pooled=True):
    """DNETFn's forward launches over S's frames; out: None (fresh tensors) or a callable handing
    out each launch's output tensors (nconv._outputs). Returns the TrainActs."""
    w4, w5, w6 = (None, None, None) if wph is None else tuple(wph)
    if pooled:
        spp = [dataclasses.replace(sp[k], mode=_lib.PLAIN) for k in (2, 3, 4)]
        if FUSE_HEAD_FWD:  # nconv1 inside nconv2's tile, nconv1's outputs written for the backward
            if w21 is None:
                w21 = head_weights(sp[0], sp[1], S, *W[0], *W[1])
            x2, c2, p2x, p2c, a2, x1, c1 = layer_forward_head(sp[0], sp[1], S, *W[0], *W[1], w21, train=True,
                                                              out=out)
        else:
            x1, c1 = layer_forward_raw(sp[0], S, None, None, None, *W[0], out=out)
            x2, c2, p2x, p2c, a2 = layer_forward_pooled(sp[1], x1, c1, None, None, *W[1], out=out, argmax=True)
        x3, c3, p3x, p3c, a3 = layer_forward_pooled(spp[0], p2x, p2c, None, None, *W[2], out=out, argmax=True)
        x4, c4, p4x, p4c, a4 = layer_forward_pooled(spp[1], p3x, p3c, None, None, *W[3], out=out, argmax=True)
        x5, c5 = layer_forward_raw(spp[2], p4x, p4c, None, None, *W[4], out=out)
        pools = (p2x, p2c, a2, p3x, p3c, a3, p4x, p4c, a4)
    else:
        x1, c1 = layer_forward_raw(sp[0], S, None, None, None, *W[0], out=out)
        x2, c2 = layer_forward_raw(sp[1], x1, c1, None, None, *W[1], out=out)
        x3, c3 = layer_forward_raw(sp[2], x2, c2, None, None, *W[2], out=out)
        x4, c4 = layer_forward_raw(sp[3], x3, c3, None, None, *W[3], out=out)
        x5, c5 = layer_forward_raw(sp[4], x4, c4, None, None, *W[4], out=out)
        pools = ()
    x6, c6 = layer_forward_raw(sp[5], x4, c4, x5, c5, *W[5], out=out, wphase=w4)
    x7, c7 = layer_forward_raw(sp[6], x3, c3, x6, c6, *W[6], out=out, wphase=w5)
    if pooled and FUSE_TAIL_FWD and w6 is not None and _exact_up(*S.shape[2:]):
        x8, c8, x9, c9 = _tail_train(sp[7], sp[8], x2, c2, x7, c7, W[7], W[8], w6, crop, out=out)
    elif crop is not None:
        raise RuntimeError("DNETFn: a cropped output needs the fused training tail")
    else:
        x8, c8 = layer_forward_raw(sp[7], x2, c2, x7, c7, *W[7], out=out, wphase=w6)
        x9, c9 = layer_forward_raw(sp[8], x8, c8, None, None, *W[8], out=out)
    return TrainActs(x1, c1, x2, c2, x3, c3, x4, c4, x5, c5, x6, c6, x7, c7, x8, c8, x9, c9, *pools)


class DNETFn(torch.autograd.Function):
    """Autograd node of the whole 9-layer DNET graph (training path). The backward runs the layer
    backwards in reverse order itself. Inputs: specs, capture (dict or None), crop, S, then
    DNETArgs.flatten(); outputs: nconv7's (uncropped) y, cout.

    crop: None, or DNET's output size (h, w) when the fused training tail writes nconv7's output
    already cropped (DNET._tail_crop): the outputs are then the cropped (y, cout), and the backward
    reads their gradient through the window (nconv_bwd_io tail_crop0), with no crop copy and no
    zero-padded gradient.

    Three tensors are read by two layers each (nconv2's output: down1 through the 2x2 max-pool and
    nconv6; down1's: down2 and nconv5; down2's: down3 and nconv4). With exact-fp32 forward and
    backward (the default) the pool is materialised: nconv2 / down1 / down2 write their pooled
    outputs and the pooling argmax codes in the same launch (nconv_fwd_pooled), the down layers read
    the pooled copies with plain loads, their input gradients stay pooled-sized, and each producer's
    backward adds them to the other consumer's full-resolution gradient at the argmax while forming
    {gN, gD} (nconv_bwd_ex) -- no full-resolution read-modify-write and no argmax recomputation.
    With a bf16 backward the down layers pool while loading and their input gradients are added
    into the full-resolution gradient (NCONV_BWD_ACCUMULATE)."""

    @staticmethod
    def forward(ctx, specs, capture, crop, S, *p):
        """p: DNETArgs.flatten()."""
        return DNETFn._forward(ctx, False, specs, capture, crop, S, *p)

    @staticmethod
    def _forward(ctx, train_conf, specs, capture, crop, S, *p):
        """train_conf: the output confidence is differentiable too (DNETConfFn); False leaves the
        graph, its saved tensors and its launches as DNET.forward builds them."""
        W, wph, w21, ctx.wbox = DNETArgs.unflatten(p)
        sp = specs
        pooled = _materialise_pool(S)
        ctx.crop = crop
        B = S.shape[0]
        nst = max(1, min(int(TRAIN_FWD_STREAMS), B))
        if (pooled and FUSE_HEAD_FWD and FUSE_TAIL_FWD and wph is not None and nst > 1 and
                _exact_up(*S.shape[2:])):
            # the batch in nst slices, one stream each, every launch writing its rows of full-batch
            # tensors (allocated by the first slice's launches, on this stream): the slices' kernels
            # overlap as the inference split's do; each frame's arithmetic is unchanged (bitwise the
            # one-stream pass)
            if w21 is None:
                w21 = head_weights(sp[0], sp[1], S, *W[0], *W[1])
            full = []

            def chain(b0, b1):  # (only the first slice's views are needed to name the full tensors)
                r = _train_fwd_chain(sp, W, S[b0:b1], w21, wph, crop, _batch_rows(full, B, b0, b1))
                return r if b0 == 0 else None
            res = _streams.fork_join("train_fwd", S.device, [B * k // nst for k in range(nst + 1)], chain)[0]
            base = {t.data_ptr(): t for t in full}
            acts = TrainActs(*[base[t.data_ptr()] for t in res])
        else:
            acts = _train_fwd_chain(sp, W, S, w21, wph, crop, None, pooled=pooled)
        if capture is not None:  # the three pooling stages' inputs (DNET.capture)
            capture.update(down1=(acts.x2.detach(), acts.c2.detach()), down2=(acts.x3.detach(), acts.c3.detach()),
                           down3=(acts.x4.detach(), acts.c4.detach()))
        ctx.specs = specs
        ctx.pooled = pooled
        ctx.save_for_backward(S, *p[:3 * len(LAYERS)], *acts.flatten())
        if not train_conf:
            ctx.mark_non_differentiable(acts.c9)
        ctx.set_materialize_grads(False)  # no zero-filled gradient for a c9 (or x9) that is never used
        return acts.x9, acts.c9

    @staticmethod
    def backward(ctx, g9, gc9):
        S, *saved = ctx.saved_tensors
        nw = 3 * len(LAYERS)
        A = TrainActs(*saved[nw:])
        y1, y2, yd1, yd2, yd3, y4, y5, y6, y7 = A.outputs()  # each layer's output (x, c), by layer
        if g9 is None:  # (grads are not materialised)
            g9 = torch.zeros_like(A.x9)
        if gc9 is not None:  # (DNETConfFn only; the unfused branch hands it to nconv7's general backward)
            gc9 = gc9.contiguous()
        box4, box5, box6 = (None, None, None) if ctx.wbox is None else tuple(ctx.wbox)
        need_S, *need = ctx.needs_input_grad[3:]  # (after specs, capture, crop: S, then w1, b1, s1, w2, ...)
        e, none = torch.empty_like, (None, None)
        grad_of = lambda y: (e(y[0]), e(y[1]))  # noqa: E731  an (x, c) pair's gradient (gx, gc), to be overwritten
        layers = [_BwdLayer(sp, w, b, s, e(w) if need[3 * i] else None, e(b) if need[3 * i + 1] else None)
                  for i, (sp, (w, b, s)) in enumerate(zip(ctx.specs, DNETArgs.unflatten(saved[:nw]).layers))]
        n1, n2, d1, d2, d3, n4, n5, n6, n7 = layers
        pooled = ctx.pooled
        red = WgradReduce()  # every layer's weight-gradient reduction in two launches at the end
        side = _streams.SideStream("dnet_wgrad", S.device) if (pooled and WGRAD_STREAM) else None

        def split(spec, inputs, y, co, gy, gco, gin, gw, gb, head=None, tail=None, **kw):
            # the weight gradient runs on the side stream, concurrent with this layer's input gradient
            # (and the next layers' input gradients, which do not depend on it): it needs only tensors
            # that are complete when this layer's backward starts
            if side is None or (gw is None and gb is None):
                layer_backward(spec, inputs, y, co, gy, gco, gin, gw, gb, defer=red, head=head, tail=tail, **kw)
                return
            st = side.fork()
            layer_backward(spec, inputs, y, co, gy, gco, gin, None, None, defer=red, head=head,
                           tail=None if tail is None else tail._replace(gw=None), **kw)  # (no gw7)
            with torch.cuda.stream(st):
                layer_backward(spec, inputs, y, co, gy, gco, InputGrads(), gw, gb, defer=red, tail=tail, **kw)

        def bwd(layer, a, b, out, gout, into_a, into_b, spec=None, **kw):
            # `layer` read the (x, c) pairs a and b and wrote out, whose gradient is gout; a's and b's gradients
            # go into the pairs into_a and into_b
            split(spec or layer.spec, layer.operands(a, b), *out, *gout, InputGrads(*into_a, *into_b), layer.gw,
                  layer.gb, **kw)

        # -- tail: nconv7, nconv6 --
        g2, g5 = grad_of(y2), grad_of(y5)
        # (nconv7's weight gradient is accumulated inside nconv6's weight-gradient pass, so the fused
        # form needs nconv6's gw or gb too; gc9, the output confidence's gradient, is None unless a
        # confidence loss was applied to forward_with_confidence's pair)
        if ctx.crop is not None or (FUSE_TAIL_BWD and pooled and _exact_up(*S.shape[2:]) and n7.gw is not None
                                    and (n6.gw is not None or n6.gb is not None)):
            # nconv7's backward inside nconv6's (nconv_bwd_ex tail): its input gradient never reaches
            # HBM; its bias gradient is the sum of its output gradient (every output pixel, padding ring
            # included, as autograd's conv bias gradient), summed by the batched reduction. With the
            # cropped output nconv7's planes are the crop window from grid row / column 1
            # (step1.py:94); the gradient outside it is 0
            g9c = g9.contiguous()
            bwd(n6, y2, y5, y6, none, g2, g5, box=box6,
                tail=TailBwd(n7.spec, n7.weight, n7.bias, n7.wsum, *y7, g9c, n7.gw,
                             crop0=None if ctx.crop is None else 1, gcout=gc9))
            if n7.gb is not None:
                red.add_sum(g9c, n7.gb)
        else:
            g6 = grad_of(y6)
            bwd(n7, y6, none, y7, (g9, gc9), g6, none)
            bwd(n6, y2, y5, y6, g6, g2, g5)             # nconv2's output (overwrite) + up
        # -- up: nconv5 (down1's output + up), nconv4 (down2's output + up) --
        gd1, g4 = grad_of(yd1), grad_of(y4)
        bwd(n5, yd1, y4, y5, g5, gd1, g4, box=box5)
        gd2, gd3 = grad_of(yd2), grad_of(yd3)
        bwd(n4, yd2, yd3, y4, g4, gd2, gd3, box=box4)
        # -- down: down3, down2, down1 --
        if pooled:  # each reads its producer's pooled copy; its pooled-sized input gradient is routed
            # into the producer's output gradient by the producer's own backward (pool_grad)
            p2, p3, p4 = (A.p2x, A.p2c), (A.p3x, A.p3c), (A.p4x, A.p4c)
            plain = lambda layer: dataclasses.replace(layer.spec, mode=_lib.PLAIN)  # noqa: E731
            gp4 = grad_of(p4)
            bwd(d3, p4, none, yd3, gd3, gp4, none, spec=plain(d3))
            gp3 = grad_of(p3)
            bwd(d2, p3, none, yd2, gd2, gp3, none, spec=plain(d2), pool_grad=PoolGrad(*gp4, A.a4))
            gp2 = grad_of(p2)
            bwd(d1, p2, none, yd1, gd1, gp2, none, spec=plain(d1), pool_grad=PoolGrad(*gp3, A.a3))
        else:  # each pools while loading and adds into its producer's output gradient
            bwd(d3, yd2, none, yd3, gd3, gd2, none, accumulate=True)
            bwd(d2, yd1, none, yd2, gd2, gd1, none, accumulate=True)
            bwd(d1, y2, none, yd1, gd1, g2, none, accumulate=True)
        # -- head: nconv2, nconv1 --
        # nconv2's input gradient feeds nconv1's weight gradient in-tile: nconv1's backward inside nconv2's
        head_bwd = pooled and FUSE_HEAD_BWD and not need_S
        gS = e(S) if need_S else None
        if head_bwd:
            args = (n2.spec, n2.operands(y1, none), *y2, *g2, InputGrads(), n2.gw, n2.gb)
            kw = dict(pool_grad=PoolGrad(*gp2, A.a2),
                      head=HeadBwd(n1.spec, S, n1.weight, n1.bias, n1.wsum, n1.gw, n1.gb))
            if WGRAD_LAST_MAIN:  # the last layer's weight gradient after its input gradient, on this stream
                layer_backward(*args, defer=red, **kw)
            else:
                split(*args, **kw)
        else:
            g1 = grad_of(y1)
            bwd(n2, y1, none, y2, g2, g1, none, pool_grad=PoolGrad(*gp2, A.a2) if pooled else None)
            bwd(n1, (S, None), none, y1, g1, (gS, None), none)  # (threshold: c0 has no gradient)
        # -- the reduction --
        if side is not None:
            side.join()  # (the side stream's workspaces are handed over by WgradReduce.run)
        red.run(S.device)
        grads = itertools.chain.from_iterable((layer.gw, layer.gb, None) for layer in layers)
        return (None, None, None, gS, *grads, None, None, None)  # (specs, capture, crop, S, layers, wph, w21, wbox)


class DNETConfFn(DNETFn):
    """DNETFn with a differentiable output confidence (DNET.forward_with_confidence under autograd):
    the same forward launches; the backward takes the confidence's gradient gc9 into nconv7's backward
    -- the fused tail's extra plane (nconv_bwd_tail_conf) or the general layer backward's gcout."""

    @staticmethod
    def forward(ctx, specs, capture, crop, S, *p):
        return DNETFn._forward(ctx, True, specs, capture, crop, S, *p)


def _tail_train(sp6, sp7, x2, c2, x7, c7, W6, W7, w6, crop=None, out=None):
    """nconv6 + nconv7 in one phase-tail launch writing nconv6's outputs and nconv7's whole
    (uncropped) output grid -- what the training backward reads (nconv_fwd_tail, crop0 = 0) -- or,
    with crop = (h, w), nconv7's output cropped as step1.py:94 (crop0 = 1). out: None or a callable
    as nconv._outputs takes."""
    return nconv.layer_forward_tail(sp6, sp7, x2, c2, x7, c7, W6, W7, w6, out=out, crop0=0 if crop is None else 1,
                                    size=None if crop is None else tuple(crop))


class CropFn(torch.autograd.Function):
    """xo[:, :, 1:1+h, 1:1+w] (step1.py:94); its backward zero-pads the gradient in one launch
    (autograd's two slice backwards zero-fill and copy twice). The crop is returned as a fresh
    tensor (not a view, as the reference's slice is), so in-place operations on DNET's output
    (clamp_, masked_fill_, ...) stay legal under autograd; the copy is the output's size only."""

    @staticmethod
    def forward(ctx, x, h, w):
        ctx.pad = (1, x.shape[3] - 1 - w, 1, x.shape[2] - 1 - h)
        return x[:, :, 1:1 + h, 1:1 + w].contiguous()

    @staticmethod
    def backward(ctx, g):
        return torch.nn.functional.pad(g, ctx.pad), None, None


def _materialise_pool(S):
    """The training graph's pooled form (DNETFn): both arithmetics exact fp32 and every pooled
    level at least 2x2 (nconv_fwd_pooled / the pooled-gradient backward are built for that)."""
    return (nconv.FORWARD_MATH == _lib.MATH_FP32 and nconv.BACKWARD_MATH == _lib.MATH_FP32 and
            min(S.shape[2], S.shape[3]) >= 16)


def crop_hw(H, W, crop):
    """Output size after nconv7 (grid (H+2) x (W+2)) and the crop of step1.py:94."""
    if crop == "literal":
        return max(0, min(481, H + 2) - 1), max(0, min(641, W + 2) - 1)
    if crop == "generalized":
        return H, W
    raise ValueError(f"crop must be 'literal' or 'generalized', got {crop!r}")


class DNET(nn.Module):
    """NConv U-Net (step1.py:30-94). `out_ch` is accepted and ignored like the reference (:19,31,36).

    crop='literal' reproduces xout[:, :, 1:481, 1:641] (e.g. 353x640 at 352x1216 input);
    crop='generalized' returns [1:H+1, 1:W+1], identical to literal at 480x640.
    """

    def __init__(self, out_ch, crop="literal"):
        super().__init__()
        pos_fn = "softplus"
        num_channels = 8
        self.crop = crop
        self.nconv1 = NConv2d(1, num_channels, (5, 5), pos_fn, "p", padding=(2, 2))
        self.nconv2 = NConv2d(num_channels, num_channels, (5, 5), pos_fn, "p", padding=(2, 2))
        self.nconv_down1 = NConv2d(num_channels, num_channels, (5, 5), pos_fn, "p", padding=(2, 2))
        self.nconv_down2 = NConv2d(num_channels, num_channels, (5, 5), pos_fn, "p", padding=(2, 2))
        self.nconv_down3 = NConv2d(num_channels, num_channels, (5, 5), pos_fn, "p", padding=(2, 2))
        self.nconv4 = NConv2d(2 * num_channels, num_channels, (3, 3), pos_fn, "p", padding=(1, 1))
        self.nconv5 = NConv2d(2 * num_channels, num_channels, (3, 3), pos_fn, "p", padding=(1, 1))
        self.nconv6 = NConv2d(2 * num_channels, num_channels, (3, 3), pos_fn, "p", padding=(0, 0))
        self.nconv7 = NConv2d(num_channels, 1, (1, 1), pos_fn, "k")
        # Set to a dict to receive the (x, c) inputs of the three pooling stages on the next
        # forward (diagnostics / tests); None in normal use.
        self.capture = None

    # Training path: one autograd node for the whole graph (DNETFn, gradients of shared tensors
    # accumulated in-kernel); False: one node per layer (NConvLayerFn), for comparison.
    whole_graph_autograd = True

    # -- hooks ----------------------------------------------------------------------------------
    def _prologue(self, layers, S):
        """Run each layer's forward pre-hooks (EnforcePos) and compute s[o] for every layer."""
        batched_sp, weights = [], []
        for m in layers:
            kind, usable = _layer_class(m)
            if kind == "foreign":
                for h in list(m._forward_pre_hooks.values()):
                    h(m, (S,))
                usable = _layer_class(m)[1]  # (a hook may have replaced the weight)
            if not usable:
                raise RuntimeError(f"{type(m).__name__}.weight must be a contiguous fp32 device tensor")
            weights.append(m.weight.data)
            batched_sp.append(kind == "ours" and m.training)
        wsums = _wsum_views(weights, S.device)
        weight_prep(weights, batched_sp, wsums)
        return wsums

    def _merged_prologue_layers(self, layers, training):
        """The layers' softplus flags for a one-launch prologue, or None where the separate path must
        run: merged_prologue off, a forward pre-hook other than this package's softplus EnforcePos, a
        weight that is not a contiguous fp32 device tensor, or (training False) a layer in training mode."""
        if not self.merged_prologue:
            return None
        flags = []
        for m in layers:
            kind, usable = _layer_class(m)
            if kind == "foreign" or not usable or (m.training and not training):
                return None
            flags.append(kind == "ours" and m.training)
        return flags

    def _phase_layers_ok(self):
        """nconv4/5/6 run in the phase form: phase_upcat on, the exact-fp32 forward, and the three
        layers 16 -> 8 channels 3x3 (the phase-weight kernels' geometry)."""
        return self.phase_upcat and nconv.FORWARD_MATH == _lib.MATH_FP32 and all(
            tuple(m.weight.shape) == (8, 16, 3, 3) for m in (self.nconv4, self.nconv5, self.nconv6))

    def _train_prologue(self, layers, S):
        """(wsums, phase weights, head weights, box weights) of the whole-graph training pass from
        one nconv_train_prologue launch (EnforcePos applied in place first, as the hooks would),
        or None where the separate path must run: merged_prologue off, a forward pre-hook other
        than this package's softplus EnforcePos, weights that are not contiguous fp32 device
        tensors, or a matrix-core arithmetic. Phase / box weights are None when phase_upcat is off
        or the UpCat layers do not have the phase form's geometry; head weights None when the
        fused training head is off."""
        if nconv.FORWARD_MATH != _lib.MATH_FP32 or not _materialise_pool(S):
            return None
        sp = self._merged_prologue_layers(layers, training=True)
        if sp is None:
            return None
        dev = S.device
        weights = [m.weight.data for m in layers]
        wsums = _wsum_views(weights, dev)
        head, w21 = None, None
        if FUSE_HEAD_FWD and self._head_shapes(layers[0], layers[1]):
            w21 = torch.empty(nconv.HEAD_WEIGHTS_FLOATS, device=dev, dtype=torch.float32)
            head = (0, 1, w21, nconv.sync_counter(dev))
        phase, wph, wbox = None, None, None
        if self._phase_layers_ok():
            wph = torch.empty((3, 1024), device=dev, dtype=torch.float32)
            wbox = torch.empty((3, nconv.BOX_WEIGHT_FLOATS), device=dev, dtype=torch.float32)
            phase = ([5, 6, 7], [8, 8, 0], list(wph), list(wbox))
        train_prologue(weights, sp, wsums, head=head, phase=phase)
        return wsums, wph, w21, wbox

    # The whole-graph training pass writes DNET's cropped output from the fused tail where it can
    # (_tail_crop); False: nconv7's whole grid, then CropFn (tests compare the two).
    crop_in_tail = True

    def _tail_crop(self, S, wph):
        """Whether the whole-graph training pass writes DNET's cropped output straight from the
        fused tail (no crop copy, no zero-padded gradient): the pooled graph with the fused
        training tail and its backward, exactly-2x UpCat, a crop window covering every nconv6 pixel
        (crop0 = 1 <= nconv7's padding, the window at least (H - 1) x (W - 1): the generalized crop,
        or the literal one up to 481 x 641), and nconv7's weight gradient only with nconv6's
        (it is accumulated in nconv6's weight-gradient pass)."""
        H, W = S.shape[2], S.shape[3]
        oh, ow = crop_hw(H, W, self.crop)
        l6, l7 = self.nconv6, self.nconv7
        return (self.crop_in_tail and wph is not None and FUSE_TAIL_FWD and FUSE_TAIL_BWD and _materialise_pool(S)
                and _exact_up(H, W) and tuple(l7.padding) == (2, 2) and oh >= H - 1 and ow >= W - 1
                and (not l7.weight.requires_grad or l6.weight.requires_grad or l6.bias.requires_grad))

    # The eval-mode forward builds its weight-only prologue -- the normalisers, the exact head's
    # composed weights and nconv4/5/6's phase weights -- in one launch (nconv_weight_prologue,
    # bitwise the three separate launches); False: the separate launches.
    merged_prologue = True

    def _eval_prologue(self, layers, S):
        """(wsums, phase weights or None, head weights or None) from one nconv_weight_prologue launch, or None where the separate path must run: merged_prologue off,
        a layer in training mode (EnforcePos then rewrites the weights first), a forward pre-hook
        other than this package's EnforcePos, or weights that are not contiguous fp32 device
        tensors."""
        if self._merged_prologue_layers(layers, training=False) is None:
            return None
        dev = S.device
        weights = [m.weight.data for m in layers]
        wsums = _wsum_views(weights, dev)
        head, w21 = None, None
        l1, l2 = layers[0], layers[1]
        if nconv.FORWARD_MATH == _lib.MATH_FP32 and self._use_head(l1, l2):
            w21 = torch.empty(nconv.HEAD_WEIGHTS_FLOATS, device=dev, dtype=torch.float32)
            head = (l1.weight.data, l2.weight.data, w21)
        phase, wph = None, None
        if self._phase_layers_ok():  # (their weights are contiguous: they are among `layers`)
            wph = torch.empty((3, 1024), device=dev, dtype=torch.float32)
            phase = ([m.weight.data for m in (self.nconv4, self.nconv5, self.nconv6)], [8, 8, 0], list(wph))
        nconv.weight_prologue(weights, wsums, head=head, phase=phase)
        return wsums, wph, w21

    # -- forward ----------------------------------------------------------------------------------
    def forward(self, S):
        if export.is_exporting():  # the export graph: the reference's own ops (export.py)
            return export.dnet(self, S)
        S = self._checked_input(S, "DNET.forward")
        layers = [getattr(self, n) for n in LAYERS]
        grad = self._records_grad(S)
        H, W = S.shape[2], S.shape[3]
        out_h, out_w = crop_hw(H, W, self.crop)
        if not grad and min(H, W) >= 16:
            return self._inference(S, layers, False)[0]

        (l1, l2, d1, d2, d3, l4, l5, l6, l7) = layers
        if grad and self.whole_graph_autograd and S.shape[0] > 0:
            return self._whole_graph(S, layers, DNETFn)[0]

        wsum = self._prologue(layers, S)
        (s1, s2, sd1, sd2, sd3, s4, s5, s6, s7) = wsum
        f = nconv_layer if grad else (lambda spec, *a, wphase=None: layer_forward_raw(spec, *a, wphase=wphase))

        wph = self._phase_weights(S.device)
        w4, w5, w6 = (None, None, None) if wph is None else tuple(wph)

        x1, c1 = f(l1.spec(_lib.THRESH, 0.01), S, None, None, None, l1.weight, l1.bias, s1)
        x1, c1 = f(l2.spec(), x1, c1, None, None, l2.weight, l2.bias, s2)
        x2, c2 = f(d1.spec(_lib.POOL2), x1, c1, None, None, d1.weight, d1.bias, sd1)
        x3, c3 = f(d2.spec(_lib.POOL2), x2, c2, None, None, d2.weight, d2.bias, sd2)
        x4, c4 = f(d3.spec(_lib.POOL2), x3, c3, None, None, d3.weight, d3.bias, sd3)
        if self.capture is not None:
            self.capture.update(down1=(x1.detach(), c1.detach()), down2=(x2.detach(), c2.detach()),
                                down3=(x3.detach(), c3.detach()))
        x34, c34 = f(l4.spec(_lib.UPCAT_SKIP_FIRST), x3, c3, x4, c4, l4.weight, l4.bias, s4, wphase=w4)
        x23, c23 = f(l5.spec(_lib.UPCAT_SKIP_FIRST), x2, c2, x34, c34, l5.weight, l5.bias, s5, wphase=w5)
        xo, co = f(l6.spec(_lib.UPCAT_UP_FIRST), x1, c1, x23, c23, l6.weight, l6.bias, s6, wphase=w6)
        xo, co = f(l7.spec(), xo, co, None, None, l7.weight, l7.bias, s7)
        return xo[:, :, 1:1 + out_h, 1:1 + out_w]

    def _whole_graph(self, S, layers, fn):
        """(depth, confidence) of the whole-graph training pass, fn = DNETFn (the confidence is not
        differentiable: forward drops it) or DNETConfFn; cropped by the fused tail where it can
        (_tail_crop), else by CropFn, the confidence by the same window."""
        (l1, l2, d1, d2, d3, l4, l5, l6, l7) = layers
        out_h, out_w = crop_hw(S.shape[2], S.shape[3], self.crop)
        specs = (l1.spec(_lib.THRESH, 0.01), l2.spec(), d1.spec(_lib.POOL2), d2.spec(_lib.POOL2),
                 d3.spec(_lib.POOL2), l4.spec(_lib.UPCAT_SKIP_FIRST), l5.spec(_lib.UPCAT_SKIP_FIRST),
                 l6.spec(_lib.UPCAT_UP_FIRST), l7.spec())
        wsum, wph, w21, wbox = self._train_prologue(layers, S) or \
            (self._prologue(layers, S), self._phase_weights(S.device), None, None)
        args = DNETArgs(tuple((m_.weight, m_.bias, s_) for m_, s_ in zip(layers, wsum)), wph, w21, wbox)
        crop = (out_h, out_w) if self._tail_crop(S, wph) else None
        xo, co = fn.apply(specs, self.capture, crop, S, *args.flatten())
        if crop is not None:
            return xo, co
        return CropFn.apply(xo, out_h, out_w), (CropFn.apply(co, out_h, out_w) if fn is DNETConfFn else None)

    def forward_with_confidence(self, S):
        """(depth, confidence), both (B, 1, out_h, out_w): forward(S)'s prediction, bit for bit,
        and the confidence nconv7 propagates beside it (step1.py:92 computes it, :94 drops it),
        cropped like the depth; 0 where the crop reaches nconv7's zero border.

        Without autograd it takes the fused inference path (nconv_fwd_tail writes both), which needs
        min(H, W) >= 16. In training mode, where gradients are recorded, it takes forward's
        whole-graph training pass (the same launches, the same crop path) and both outputs are
        differentiable: a loss on the confidence (train.ConfidenceLoss) reaches every layer. A model
        in eval mode that would record gradients, or a CPU input, is refused as before."""
        if self._records_grad(S):
            if not (self.training and torch.is_tensor(S) and S.is_cuda):
                raise RuntimeError("DNET.forward_with_confidence is inference only outside training mode: call it "
                                   "under torch.no_grad(), or in training mode (train()) on a device input for a "
                                   "differentiable confidence")
            S = self._checked_input(S, "DNET.forward_with_confidence")
            if not self.whole_graph_autograd or S.shape[0] == 0:
                raise RuntimeError("DNET.forward_with_confidence under autograd needs the whole-graph training pass "
                                   "(whole_graph_autograd) and a non-empty batch")
            return self._whole_graph(S, [getattr(self, n) for n in LAYERS], DNETConfFn)
        S = self._checked_input(S, "DNET.forward_with_confidence")
        H, W = S.shape[2], S.shape[3]
        if min(H, W) < 16:
            raise ValueError(f"DNET.forward_with_confidence needs min(H, W) >= 16 (the fused inference path), got "
                             f"{H} x {W}")
        return self._inference(S, [getattr(self, n) for n in LAYERS], True)

    # -- inference ------------------------------------------------------------------------------
    def _records_grad(self, S):
        return torch.is_grad_enabled() and (S.requires_grad or any(p.requires_grad for p in self.parameters()))

    @staticmethod
    def _checked_input(S, what):
        """S as the kernels read it: a contiguous fp32 (B, 1, H, W) device tensor, or an error."""
        _require_device(S, what)
        if S.dim() != 4 or S.shape[1] != 1:
            raise ValueError(f"DNET expects (B, 1, H, W) sparse depth, got {tuple(S.shape)}")
        return S.contiguous()

    def _inference(self, S, layers, confidence):
        """(depth, confidence or None) of the fused inference path on a checked S, min(H, W) >= 16: the
        one-launch eval prologue, or the separate launches where it does not apply, then the layer chain."""
        out = torch.empty((S.shape[0], 1, *crop_hw(S.shape[2], S.shape[3], self.crop)), device=S.device,
                          dtype=torch.float32)
        out_c = torch.empty_like(out) if confidence else None
        wsum, wph, w21 = self._eval_prologue(layers, S) or \
            (self._prologue(layers, S), self._phase_weights(S.device), None)
        self._infer_split(S, layers, wsum, out, wph, w21, out_c=out_c)
        return out, out_c

    # Exact-fp32 inference convolves the nearest-2x-upsampled half of nconv4/5/6's inputs at its
    # own resolution with phase weights (include/nconv.h nconv_layer.wphase; the kernel uses them
    # where the upsampling is exactly 2x); False: the 3x3 taps over the upsampled planes.
    phase_upcat = True

    def _phase_weights(self, device):
        """Phase weights of nconv4, nconv5 (cat(skip, up): up channels 8..15) and nconv6
        (cat(up, skip): 0..7) from the current weights, one launch; None when not in use."""
        if not self._phase_layers_ok():
            return None
        buf = torch.empty((3, 1024), device=device, dtype=torch.float32)
        phase_weights([m.weight for m in (self.nconv4, self.nconv5, self.nconv6)], [8, 8, 0], list(buf))
        return buf

    # Frames are independent, so the batch can be split over `inference_streams` HIP streams, each
    # running the whole layer chain on its share, so that one stream's kernels fill the partial
    # last round of the other's (and its small quarter / eighth-resolution layers overlap the other
    # share's large ones). None = automatic: 2 for the exact-fp32 kernels (B=8 352x1216: 0.616 vs
    # 0.628 ms), 1 for the matrix-core maths, whose persistent grids are sized to the chip and
    # leave no such gaps (0.507 vs 0.555 ms). A frame's result does not depend on the split.
    inference_streams = None
    # Frames per stream of the inference split, as relative shares (None = even); an uneven split
    # staggers the streams' phases so one stream's small quarter / eighth-resolution layers run
    # beside the other's full-resolution head or tail instead of beside its own small layers.
    inference_shares = None

    def _n_streams(self, B):
        return max(1, min(self._configured_streams(), B))

    def _configured_streams(self):
        n = self.inference_streams
        if n is None:
            n = 2 if nconv.FORWARD_MATH == _lib.MATH_FP32 else 1
        return int(n)

    @staticmethod
    def split_bounds(B, n, shares=None, configured=None):
        """Frame bounds [b0 = 0, b1, ..., bn = B] of an n-way inference split: even, or by the
        relative `shares` (one positive finite number per configured stream). Shares whose count
        differs from the configured stream count, or that are not all positive and finite, raise
        ValueError; when the batch is smaller than the configured count (n clamped to B) the split
        is even."""
        bounds = [B * k // n for k in range(n + 1)]
        if shares is None:
            return bounds
        sh = [float(v) for v in shares]
        want = n if configured is None else configured
        if len(sh) != want:
            raise ValueError(f"inference_shares has {len(sh)} entries for {want} inference streams")
        if not all(math.isfinite(v) and v > 0 for v in sh):
            raise ValueError(f"inference_shares must be positive and finite, got {tuple(shares)}")
        if len(sh) != n:  # batch smaller than the configured streams: even split
            return bounds
        tot, acc = sum(sh), 0.0
        for k in range(1, n):
            acc += sh[k - 1]
            bounds[k] = min(max(int(round(B * acc / tot)), bounds[k - 1]), B)
        return bounds

    def _infer_split(self, S, layers, wsum, out, wph=None, w21=None, out_c=None):
        """The inference chain on batch slices, one stream each (the weight prologue once, on the
        current stream, before the fork: a prologue per stream measured slower, 16.3-16.5 k against
        16.9-17.2 k frames/s, profiles/r5_ab_stream_prologue.log). out_c: the output confidence,
        written per slice like out (forward_with_confidence), or None."""
        B = S.shape[0]
        n = self._n_streams(B)
        bounds = self.split_bounds(B, n, self.inference_shares, self._configured_streams())
        if n == 1:
            self._infer(S, layers, wsum, out, wph, w21=w21, out_c=out_c)
            return
        _streams.fork_join("infer", S.device, bounds, lambda b0, b1: self._infer(
            S[b0:b1], layers, wsum, out[b0:b1], wph, w21=w21, out_c=None if out_c is None else out_c[b0:b1]))

    def _infer(self, S, layers, wsum, out, wph=None, w21=None, out_c=None):
        """The inference chain on the current stream: each producer also writes the pooled input
        of the next down layer, and nconv6+nconv7+crop run as one launch writing `out` (and, with
        out_c, nconv7's confidence beside it). wph: the phase weights of nconv4/5/6
        (_phase_weights) or None. w21: the exact head's weights when the prologue already built
        them (_eval_prologue), else built here."""
        (l1, l2, d1, d2, d3, l4, l5, l6, l7) = layers
        (s1, s2, sd1, sd2, sd3, s4, s5, s6, s7) = wsum
        w4, w5, w6 = (None, None, None) if wph is None else tuple(wph)
        f, fp = layer_forward_raw, layer_forward_pooled
        if self._use_head(l1, l2):
            # nconv1 inside nconv2's staging: its 8-channel output never reaches HBM
            sp1, sp2 = l1.spec(_lib.THRESH, 0.01), l2.spec()
            if w21 is None and nconv.FORWARD_MATH == _lib.MATH_FP32:  # the exact head's composed weights
                w21 = head_weights(sp1, sp2, S, l1.weight, l1.bias, s1, l2.weight, l2.bias, s2)
            x1, c1, p1, q1 = layer_forward_head(sp1, sp2, S, l1.weight, l1.bias, s1, l2.weight, l2.bias, s2, w21)
        else:
            x1, c1 = f(l1.spec(_lib.THRESH, 0.01), S, None, None, None, l1.weight, l1.bias, s1)
            x1, c1, p1, q1 = fp(l2.spec(), x1, c1, None, None, l2.weight, l2.bias, s2)
        x2, c2, p2, q2 = fp(d1.spec(), p1, q1, None, None, d1.weight, d1.bias, sd1)
        x3, c3, p3, q3 = fp(d2.spec(), p2, q2, None, None, d2.weight, d2.bias, sd2)
        x4, c4 = f(d3.spec(), p3, q3, None, None, d3.weight, d3.bias, sd3)
        x34, c34 = f(l4.spec(_lib.UPCAT_SKIP_FIRST), x3, c3, x4, c4, l4.weight, l4.bias, s4, wphase=w4)
        if self.capture is not None:
            self.capture.update(down1=(x1, c1), down2=(x2, c2), down3=(x3, c3))
        x23, c23 = f(l5.spec(_lib.UPCAT_SKIP_FIRST), x2, c2, x34, c34, l5.weight, l5.bias, s5, wphase=w5)
        self._fused_tail(l6, l7, s6, s7, x1, c1, x23, c23, out, w6, out_c=out_c)

    # Inference evaluates nconv1 inside nconv2's kernel (nconv_fwd_head) when the layers have
    # DNET's geometry -- in exact fp32 with nconv1 on the nonzero taps only and nconv2's confidence
    # mass from composed weights (include/nconv.h nconv_fwd_head); set False to run them as two
    # launches.
    fused_head = True

    def _use_head(self, l1, l2):
        return self.fused_head and self._head_shapes(l1, l2)

    @staticmethod
    def _head_shapes(l1, l2):
        return (l1.in_channels, l1.out_channels, tuple(l1.kernel_size), tuple(l1.padding), tuple(l1.stride)) == \
            (1, 8, (5, 5), (2, 2), (1, 1)) and \
            (l2.in_channels, l2.out_channels, tuple(l2.kernel_size), tuple(l2.padding), tuple(l2.stride)) == \
            (8, 8, (5, 5), (2, 2), (1, 1)) and tuple(l1.dilation) == (1, 1) and tuple(l2.dilation) == (1, 1) \
            and l1.groups == 1 and l2.groups == 1

    def _fused_tail(self, l6, l7, s6, s7, x1, c1, x23, c23, out, w6=None, out_c=None):
        """nconv6 + nconv7 + crop into `out` (nconv_fwd_tail); out_c (of out's shape, contiguous)
        receives nconv7's confidence at the same pixels, 0 in nconv7's zero border."""
        out_h, out_w = out.shape[2], out.shape[3]
        if out_h == 0 or out_w == 0 or out.shape[0] == 0:
            return out
        if out_c is not None and not (out_c.shape == out.shape and out_c.is_contiguous() and
                                      out_c.dtype == torch.float32 and out_c.device == out.device):
            raise RuntimeError("fused tail: out_c must be a contiguous fp32 tensor of out's shape and device")
        if tuple(l7.kernel_size) != (1, 1) or l7.padding[0] != l7.padding[1] or tuple(l7.stride) != (1, 1):
            raise RuntimeError("fused tail needs nconv7 = 1x1, stride 1, square padding")
        return nconv.layer_forward_tail(l6.spec(_lib.UPCAT_UP_FIRST), l7.spec(), x1, c1, x23, c23,
                                        (l6.weight, l6.bias, s6), (l7.weight, l7.bias, s7), w6, crop0=1, y=out,
                                        out_c=out_c)


class SETP1_NCONV(nn.Module):
    """Unguided depth network wrapper (step1.py:15-27); state_dict prefix `d_net.`.

    forward(S) -> d_net(S). Also accepts forward(depth0, depth1, ...) and runs DNET on their
    batch concatenation: the call the guided model makes (models/step2.py:62,107), which the
    reference's one-argument forward rejects with a TypeError.
    """

    def __init__(self, crop="literal"):
        super().__init__()
        self.d_net = DNET(32, crop=crop)

    def forward(self, x0_d, *more):
        if more:
            x0_d = torch.cat((x0_d,) + tuple(more), dim=0)
        return self.d_net(x0_d)

    def forward_with_confidence(self, x0_d):
        """(depth, confidence) of d_net on one batch of sparse depth (DNET.forward_with_confidence)."""
        return self.d_net.forward_with_confidence(x0_d)
