"""Helpers of the fc-action head tests: the fp64 head, small head-only graphs, and a copy of synthetic_weights' draw order from
before InnerProduct layers had weights (oracle/tsn_oracle.py's forward skips InnerProduct, so the head's reference lives here)."""
import hashlib

import numpy as np


def head_fp64(W, b, gp):
    """y = W @ gp + b per row of gp, everything promoted to fp64 first."""
    return np.asarray(gp, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64)


def head_graph(bi, k, n, cin=32, size=4):
    """data [cin, size, size] -> conv 1x1 + BN (no ReLU: signed pool values) -> global AVE pool [k] -> InnerProduct [n]."""
    g = bi.Graph("head", "data", (cin, size, size))
    g.layers.append(bi.Layer("c", "Convolution", ["data"], ["c"], k, 1, 1, 0))
    g.layers.append(bi.Layer("c_bn", "BN", ["c"], ["c_bn"]))
    g.layers.append(bi.Layer("gp", "Pooling", ["c_bn"], ["gp"], kernel=size, stride=1, pad=0, pool="AVE"))
    g.layers.append(bi.Layer("drop", "Dropout", ["gp"], ["gp"]))
    g.layers.append(bi.Layer("fc", "InnerProduct", ["gp"], ["fc"], num_output=n))
    return g


def plan_digest(plan):
    return hashlib.sha1(repr((plan.ops, plan.tensors, plan.feature_slot, plan.feature_dim, sorted(plan.blob_loc.items()))).encode()).hexdigest()


def old_synthetic_weights(graph, seed):
    """tsn/net.py:synthetic_weights as it drew before the head: one generator, graph order, nothing for InnerProduct."""
    rng = np.random.default_rng(seed)
    w = {}
    shapes = {graph.input_name: graph.input_shape[0]}
    for l in graph.layers:
        if l.type == "Convolution":
            cin = shapes[l.bottoms[0]]
            fan_in = cin * l.kernel * l.kernel
            w[l.name] = {
                "W": (rng.standard_normal((l.num_output, cin, l.kernel, l.kernel)) * np.sqrt(2.0 / fan_in)).astype(np.float32),
                "b": (rng.standard_normal(l.num_output) * 0.05).astype(np.float32)}
            shapes[l.tops[0]] = l.num_output
        elif l.type == "BN":
            c = shapes[l.bottoms[0]]
            w[l.name] = {"scale": rng.uniform(0.5, 1.5, c).astype(np.float32),
                         "shift": (rng.standard_normal(c) * 0.1).astype(np.float32),
                         "mean": (rng.standard_normal(c) * 0.1).astype(np.float32),
                         "var": rng.uniform(0.5, 1.5, c).astype(np.float32)}
            shapes[l.tops[0]] = c
        elif l.type == "Concat":
            shapes[l.tops[0]] = sum(shapes[b] for b in l.bottoms)
        elif l.type == "InnerProduct":
            shapes[l.tops[0]] = l.num_output
        else:
            shapes[l.tops[0]] = shapes[l.bottoms[0]]
    return w
