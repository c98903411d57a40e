"""fp64 reference of ONE op of a lowered TSN plan (``Graph.plan()``, the fused form the product runs), from that op's own input.

The reference is built from the graph's un-folded layers -- the ``Convolution`` W / b and the ``BN`` statistics, evaluated through
``tsn_oracle.forward`` -- never from the device's packed or BN-folded weights, so a folding or packing error shows.  Every op kind of
the fused plan has a rule:

* ``conv``: Convolution + BN (+ ReLU) of the op's layers; merged siblings (``segments``) give one output per segment, each at its own
  destination and channel offset; a ``pre_pool`` op max-pools its input (the graph's Pooling layer, fp64) before the 1x1 convolution;
  a projection with ``bias=False`` (the linear half of a commuted ``pool_proj``) is ``a * (W x)``: BN's scale, no bias, no ReLU;
* ``avgpool`` with ``bias_from``: the avg pool that finishes a commuted ``pool_proj`` -- relu(bn(conv(avgpool(x)))) with x the input
  of the linear projection it pools, i.e. the un-commuted branch of the graph;
* ``maxpool`` / ``avgpool`` / ``gavgpool``: the graph's Pooling layer.

``read(slot, coff, c)`` supplies inputs: the region [coff, coff + c) of tensor slot ``slot`` as fp64 NCHW (slot 0: the network
input).  ``check`` is the comparison the tests use for convolutions: a layer-wide and a per-output-channel bound.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List

import numpy as np

import tsn_oracle as to

LAYER_REL = 2e-5        # |d| <= LAYER_REL * max|y| over the op's output (the single-layer bound of tests/test_tsn_gpu.py)
CHANNEL_REL = 8.5e-5    # |d| <= CHANNEL_REL * max(max|y_channel|, CHANNEL_FLOOR * max|y|) per output channel, never above the layer bound
CHANNEL_FLOOR = 1e-2    # dead or nearly dead channels (post-ReLU) are measured against 1 % of the layer's maximum


@dataclass
class Output:
    name: str           # the conv layer of a segment, else the op's name
    kind: str           # conv | linear | proj_pool | maxpool | avgpool | gavgpool
    slot: int
    coff: int
    c: int
    y: np.ndarray       # fp64 NCHW


def _layers(graph) -> Dict[str, object]:
    return {l.name: l for l in graph.layers}


def _relu_of(graph, top: str):
    for l in graph.layers:
        if l.type == "ReLU" and l.bottoms == [top]:
            return l
    raise KeyError("no ReLU on %s" % top)


def _conv_bn(graph, weights, x, conv: str, bn, relu: bool, bias: bool) -> np.ndarray:
    """Convolution (+ BN, + ReLU) of the graph's own layers on x.  bias=False: the linear projection a * (W x)."""
    by = _layers(graph)
    cl = by[conv]
    chain = [cl]
    w = {conv: weights[conv]}
    top = cl.tops[0]
    if bn is not None:
        chain.append(by[bn])
        w[bn] = weights[bn]
        top = by[bn].tops[0]
    if not bias:
        if relu:
            raise ValueError("a projection without bias has no ReLU")
        w[conv] = {"W": weights[conv]["W"], "b": np.zeros_like(weights[conv]["b"])}
        if bn is not None:                                          # keep a = scale / sqrt(var + eps), drop c = shift - a * mean
            w[bn] = dict(weights[bn], shift=np.zeros_like(weights[bn]["shift"]), mean=np.zeros_like(weights[bn]["mean"]))
    elif relu:
        chain.append(_relu_of(graph, top))
    return to.forward(chain, cl.bottoms[0], w, x, keep=(top,))[top]


def _pool(graph, x, name: str) -> np.ndarray:
    l = _layers(graph)[name]
    return to.forward([l], l.bottoms[0], {}, x, keep=(l.tops[0],))[l.tops[0]]


def conv_input(graph, op, read: Callable) -> np.ndarray:
    """What a conv op multiplies: its source region, max-pooled first when the op carries a folded pool."""
    x = read(op.src, op.src_coff, op.cin)
    return _pool(graph, x, op.pre_pool[2]) if op.pre_pool else x


def producer(plan, slot: int):
    """(op, segment or None) of the plan that writes slot ``slot``."""
    for op in plan.ops:
        for sg in (op.segments or []):
            if sg.dst == slot:
                return op, sg
        if not op.segments and op.dst == slot:
            return op, None
    raise KeyError("no op writes slot %d" % slot)


def op_reference(graph, weights, plan, op, read: Callable) -> List[Output]:
    """fp64 output(s) of one op of ``plan`` from the inputs ``read`` supplies."""
    if op.kind == "conv":
        x = conv_input(graph, op, read)
        if op.segments:
            parts = [(sg.name, sg.bn, sg.relu, sg.bias, sg.dst, sg.dst_coff, sg.cout) for sg in op.segments]
        else:
            parts = [(op.name, op.bn, op.relu, op.bias, op.dst, op.dst_coff, op.cout)]
        out = []
        for name, bn, relu, bias, dst, coff, cout in parts:
            y = _conv_bn(graph, weights, x, name, bn, relu, bias)
            assert y.shape[1] == cout, (name, y.shape, cout)
            out.append(Output(name, "conv" if bias else "linear", dst, coff, cout, y))
        return out
    if op.kind == "avgpool" and op.bias_from is not None:
        lin, _ = producer(plan, op.src)                             # the linear projection this pool finishes
        x = conv_input(graph, lin, read)
        conv, bn = op.bias_from
        y = _conv_bn(graph, weights, _pool(graph, x, op.name), conv, bn, op.relu, True)
        return [Output(op.name, "proj_pool", op.dst, op.dst_coff, op.cout, y)]
    if op.kind in ("maxpool", "avgpool", "gavgpool"):
        y = _pool(graph, read(op.src, op.src_coff, op.cin), op.name)
        return [Output(op.name, op.kind, op.dst, op.dst_coff, op.cout, y)]
    raise ValueError("op kind %s has no reference" % op.kind)


def check(got: np.ndarray, want: np.ndarray, channel_rel: float = CHANNEL_REL):
    """(ok, layer ratio, channel ratio) of a convolution's output against its fp64 reference (NCHW).  The layer ratio is
    max|d| / max|y|; the channel ratio is the largest max|d_c| / max(max|y_c|, CHANNEL_FLOOR * max|y|).  ok: both within their
    bounds, where a channel's bound is never looser than the layer's."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False, np.inf, np.inf
    d = np.abs(got - want)
    ymax = np.abs(want).max()
    scale = np.maximum(np.abs(want).max(axis=(0, 2, 3)), CHANNEL_FLOOR * ymax)
    dc = d.max(axis=(0, 2, 3))
    bound = np.minimum(LAYER_REL * ymax, channel_rel * scale)
    ok = bool(np.isfinite(got).all() and d.max() <= LAYER_REL * ymax and (dc <= bound).all())
    return ok, float(d.max() / ymax), float((dc / scale).max())
