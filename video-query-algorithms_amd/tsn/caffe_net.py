"""``CaffeNet``-shaped front door for the MI355X TSN extractor.

The reference touches exactly four things of ``pyActionRecog.action_caffe.CaffeNet``:
``CaffeNet(net_proto, net_weights, device_id)`` (calcSig_wOF.py:52,55), ``predict_single_frame([frame], score_name,
frame_size=(340,256))`` (:94), ``predict_single_flow_stack(flow_stack, score_name, frame_size=(340,256))`` (:111) and
``net._net.blobs[blob].data[0]`` (:95,112).  This class offers the same four, so the reference's per-snippet loop runs
unchanged on top of it, plus ``extract_clips`` -- the batched path (all B*T crops in one forward) the drop-in
command line uses.
Built with ``scores=True`` the two ``predict_*`` methods also do what every other TSN script reads them for: they return the
``score_name`` blob of the ten over-sampled crops (crop order restated from memory).

Weights: a ``.caffemodel`` (decoded by ``tsn/caffemodel.py`` without Caffe or a protobuf schema; the BN blob order is
"parity unpinned", see there), an ``.npz`` with ``<layer>/W``, ``<layer>/b`` for convolutions and
``<layer>/scale|shift|mean|var`` for the frozen BN layers, or ``synthetic:<seed>`` (random init of the right
architecture).
"""
from __future__ import annotations

import numpy as np

from . import bn_inception, frames
from .ingest import FrameIngest
from .net import FLOW_MEAN, RGB_MEAN, TsnNet, synthetic_weights


def load_weights(graph, spec: str):
    if spec.startswith("synthetic:"):
        return synthetic_weights(graph, seed=int(spec.split(":", 1)[1]))
    if spec.endswith(".npz"):
        z = np.load(spec, allow_pickle=False)
        out = {}
        for key in z.files:
            layer, field = key.rsplit("/", 1)
            out.setdefault(layer, {})[field] = z[key]
        return out
    if spec.endswith(".caffemodel"):
        from .caffemodel import weights_from_caffemodel
        return weights_from_caffemodel(spec, graph)
    raise ValueError("weights file %r: expected .caffemodel, .npz or synthetic:<seed>" % spec)


def weights_digest(spec: str) -> str:
    """Names the CONTENT of a weights specification: ``synthetic:<seed>`` as it is, a file by a digest of its bytes."""
    if spec.startswith("synthetic:"):
        return spec
    try:                                   # 8 ms for a 41 MB .caffemodel; SHA-1 (40 ms) where the module is missing
        import xxhash
        h, tag = xxhash.xxh3_128(), "file:xxh3:"
    except ImportError:
        import hashlib
        h, tag = hashlib.sha1(), "file:"
    with open(spec, "rb") as f:
        for piece in iter(lambda: f.read(1 << 22), b""):
            h.update(piece)
    return tag + h.hexdigest()


def save_weights(path: str, weights):
    np.savez(path, **{"%s/%s" % (layer, f): a for layer, d in weights.items() for f, a in d.items()})


class _Blob:
    def __init__(self, data):
        self.data = data


class _NetView:
    def __init__(self):
        self.blobs = {}


class CaffeNet:
    def __init__(self, net_proto, net_weights, device_id=0, max_crops=96, feature_blob="global_pool", resize_rule="cv2", scores=False,
                 score_name="fc-action", host_oversample=False):
        """resize_rule: "cv2" = OpenCV's fixed-point INTER_LINEAR, what the reference's ``cv2.resize(frame, (340, 256))``
        computes (default); "exact" = exact fp64 bilinear weights (tsn/frames.py).
        scores: False (default) = the feature path: ``predict_*`` run crop 0 and return ``None``.  True = pyActionRecog's score
        interface: the plan also keeps the ``score_name`` blob, ``predict_*`` run the ten over-sampled crops (``over_sample=False``:
        crop 0 alone) through the device network and return its ``[crops][classes]`` float32 scores; ``_net.blobs`` then holds one
        row per crop of the feature blob and of the score blob.  The frame or stack is uploaded once and the ten crops are cut on the
        device (FrameIngest.oversample_from_frames); ``host_oversample=True`` cuts them with numpy and uploads the crops instead
        (tsn/frames.py:oversample*) -- the same bytes and scores either way (order and x-flow inversion restated from memory, parity
        unpinned)."""
        if resize_rule not in frames.RESIZE_RULES:
            raise ValueError("resize_rule must be 'cv2' or 'exact'")
        self._resize_rule = resize_rule
        self._graph = bn_inception.load_prototxt(net_proto) if isinstance(net_proto, str) else net_proto
        self._blob = feature_blob
        self._scores = bool(scores)
        self._host_oversample = bool(host_oversample)
        self._score_name = score_name
        keep = (score_name,) if self._scores and score_name != feature_blob else ()
        if self._scores:
            max_crops = max(max_crops, 10)
        self._channels = self._graph.input_shape[0]
        self._mean = RGB_MEAN if self._channels == 3 else tuple([128.0] * self._channels)
        if isinstance(net_weights, str):
            # read (and fold, and lay out) only if the packed form of exactly these weights is not in the cache next to the library
            graph = self._graph
            self._model = TsnNet(graph, lambda: load_weights(graph, net_weights), max_crops=max_crops, device=device_id, feature_blob=feature_blob,
                                 cache_key=weights_digest(net_weights), keep=keep)
        else:
            self._model = TsnNet(self._graph, net_weights, max_crops=max_crops, device=device_id, feature_blob=feature_blob, keep=keep)
        self._net = _NetView()
        self._ingest = FrameIngest(self._channels, device_id, resize_rule)

    # -- the reference's per-snippet interface ------------------------------------------------------------
    def _predict(self, crop0, ten, ten_dev, score_name, over_sample):
        if not self._scores:
            crops = crop0()[None]                                                                   # crop 0 of the 10-crop over-sample
            _, ps = self._model.forward(crops, 1, self._mean)
            self._net.blobs[self._blob] = _Blob(ps.reshape(1, -1, 1, 1))        # .data[0] is what calcSig reads
            return None
        name = self._score_name if score_name is None else score_name
        if name not in self._model.plan.blob_loc or (name != self._score_name and name != self._blob):
            raise KeyError("score blob %r is not computed by this extractor (built with score_name=%r, feature_blob=%r)"
                           % (name, self._score_name, self._blob))
        if over_sample and not self._host_oversample:
            crops = ten_dev()                                                   # cut on the device: the frame went up, not its ten crops
            self._ingest.sync()
            n = crops.shape[0]
            ps = np.empty((n, self._model.feature_dim), dtype=np.float32)
            self._model.forward_device(crops.data_ptr(), n, 1, self._mean, per_snippet_out=ps)
        else:
            crops = ten() if over_sample else crop0()[None]
            n = crops.shape[0]
            _, ps = self._model.forward(crops, 1, self._mean)
        self._net.blobs[self._blob] = _Blob(ps.reshape(n, -1, 1, 1))            # one row per crop; .data[0] is crop 0, as without scores
        score = ps if name == self._blob else np.ascontiguousarray(self._model.read_blob(name, n).reshape(n, -1))
        self._net.blobs[name] = _Blob(score.reshape(n, -1, 1, 1))
        return score

    def predict_single_frame(self, frame, score_name=None, over_sample=True, frame_size=(340, 256)):
        return self._predict(lambda: frames.crop0(frame[0], frame_size, rule=self._resize_rule),
                             lambda: frames.oversample(frame[0], frame_size, rule=self._resize_rule),
                             lambda: self._ingest.oversample_from_frames(np.asarray(frame[0])[None], frame_size), score_name, over_sample)

    def predict_single_flow_stack(self, frame, score_name=None, over_sample=True, frame_size=(340, 256)):
        return self._predict(lambda: np.stack([frames.crop0(f, frame_size, rule=self._resize_rule) for f in frame], axis=-1),
                             lambda: frames.oversample_flow_stack(frame, frame_size, rule=self._resize_rule),
                             lambda: self._ingest.oversample_from_frames(np.stack(frame)[None], frame_size), score_name, over_sample)

    # -- the batched path ------------------------------------------------------------------------------------
    def extract_clips(self, crops: np.ndarray, T: int, on_device: bool = False):
        """crops uint8 [B*T, 224, 224, C] -> consensus features [B, D] float64 (calcSig_wOF.py:82); with
        ``on_device`` a torch tensor that never left the GPU (the block a rank contributes to the all-gather)."""
        out = []
        per = (self._model.max_crops // T) * T
        if per == 0:
            raise ValueError("max_crops (%d) is smaller than T (%d)" % (self._model.max_crops, T))
        for i in range(0, crops.shape[0], per):
            if on_device:
                import torch
                chunk = torch.from_numpy(np.ascontiguousarray(crops[i:i + per], dtype=np.uint8)).to(torch.device("cuda", self._model.device))
                self._model.forward_device(chunk.data_ptr(), chunk.shape[0], T, self._mean)
                out.append(self._model.features_tensor(chunk.shape[0] // T).clone())
            else:
                feat, _ = self._model.forward(crops[i:i + per], T, self._mean, want_per_snippet=False)
                out.append(feat)
        if on_device:
            import torch
            return torch.cat(out, dim=0)
        return np.concatenate(out, axis=0)

    def _per_forward(self, T: int, over_sample: bool):
        """(snippets per forward, the T the forward runs with): with ``over_sample`` every snippet is ten crops, snippet-major, and
        the consensus over T' = 10 T of them is the average over snippets x crops."""
        Tf = 10 * T if over_sample else T
        per = (self._model.max_crops // Tf) * T
        if per == 0:
            raise ValueError("max_crops (%d) is smaller than %s (%d)" % (self._model.max_crops, "10 T" if over_sample else "T", Tf))
        return per, Tf

    def crops_from_frames(self, frames_: np.ndarray, frame_size=(340, 256), crop=224):
        """Decoded frames -> device crops; see :class:`tsn.ingest.FrameIngest` (this extractor's own instance)."""
        return self._ingest.crops_from_frames(frames_, frame_size, crop)

    def sync_ingest(self):
        self._ingest.sync()

    def crops_from_jpegs(self, files, frame_size=(340, 256), crop=224, lane=0):
        """JPEG file contents -> device crops; see :class:`tsn.ingest.FrameIngest`."""
        return self._ingest.crops_from_jpegs(files, frame_size, crop, lane)

    def oversample_from_frames(self, frames_: np.ndarray, frame_size=(340, 256), crop=224):
        """Decoded frames -> the ten device crops of every snippet; see :class:`tsn.ingest.FrameIngest`."""
        return self._ingest.oversample_from_frames(frames_, frame_size, crop)

    def oversample_from_jpegs(self, files, frame_size=(340, 256), crop=224, lane=0):
        """JPEG file contents -> the ten device crops of every snippet; see :class:`tsn.ingest.FrameIngest`."""
        return self._ingest.oversample_from_jpegs(files, frame_size, crop, lane)

    def _extract_batched(self, source: str, items, per_snip: int, T: int, frame_size, on_device: bool, over_sample: bool):
        """The loop of extract_clips_from_jpegs / _from_frames (``source``: "jpegs" / "frames"): the device crops of a forward's snippets,
        ``per_snip`` items each, from crops_from_<source> or oversample_from_<source>."""
        produce = getattr(self, ("oversample_from_" if over_sample else "crops_from_") + source)
        from . import devmem
        per, T = self._per_forward(T, over_sample)
        out = []
        for i in range(0, len(items) // per_snip, per):
            crops = produce(items[i * per_snip:(i + per) * per_snip], frame_size)
            devmem.synchronize_current(self._model.device)
            nb = crops.shape[0]
            if on_device:
                self._model.forward_device(crops.data_ptr(), nb, T, self._mean)
                out.append(self._model.features_tensor(nb // T).clone())
            else:
                out.append(self._model.forward_device(crops.data_ptr(), nb, T, self._mean, np.empty((nb // T, self._model.feature_dim), dtype=np.float64)))
        if on_device:
            import torch
            return torch.cat(out, dim=0)
        return np.concatenate(out, axis=0)

    def extract_clips_from_jpegs(self, files, T: int, frame_size=(340, 256), on_device: bool = False, over_sample: bool = False):
        """JPEG file contents of B*T snippets (flow: * C planes) -> consensus features [B, D]; see crops_from_jpegs.  ``over_sample``:
        the ten crops of every snippet (oversample_from_jpegs), averaged with the snippets (see extract_clips_from_frames)."""
        return self._extract_batched("jpegs", files, 1 if self._channels == 3 else self._channels, T, frame_size, on_device, over_sample)

    def extract_clips_from_crops(self, crops, T: int, on_device: bool = False, over_sample: bool = False):
        """Device crops (torch uint8 [B*T, crop, crop, C], e.g. from ``crops_from_jpegs`` run by another thread for the NEXT batch while
        this one is in the network) -> consensus features [B, D].  ``over_sample``: the crops are the [B*T*10, ...] of
        ``oversample_from_*`` and the consensus runs over the 10 T crops of a clip."""
        nb = crops.shape[0]
        if over_sample:
            T = 10 * T
        if nb > self._model.max_crops or nb % T:
            raise ValueError("%d crops: at most max_crops (%d), a multiple of T (%d)" % (nb, self._model.max_crops, T))
        if on_device:
            self._model.forward_device(crops.data_ptr(), nb, T, self._mean)
            return self._model.features_tensor(nb // T).clone()
        # the features come back behind the forward on the extractor's own stream: the call does not wait for the decode kernels of the
        # batches ahead, which other threads have in flight on the ingest streams
        return self._model.forward_device(crops.data_ptr(), nb, T, self._mean, np.empty((nb // T, self._model.feature_dim), dtype=np.float64))

    def extract_clips_from_frames(self, frames_: np.ndarray, T: int, frame_size=(340, 256), on_device: bool = False, over_sample: bool = False):
        """Decoded frames of B*T snippets -> consensus features [B, D]: resize + crop 0 on the device, then the
        batched forward on the resident crops (no host-side image processing at all).  ``on_device``: see extract_clips.
        ``over_sample``: every snippet contributes its ten over-sampled crops (cut on the device, snippet-major) and the forward runs
        with T' = 10 T, max_crops // (10 T) clips at a time: the fp64 average over snippets x crops -- the ten-crop feature under
        ``global_pool``, the video-level class scores of the TSN test protocol under ``fc-action``."""
        return self._extract_batched("frames", frames_, 1, T, frame_size, on_device, over_sample)

    @property
    def feature_dim(self):
        return self._model.feature_dim

    def close(self):
        self._ingest.close()
        self._model.close()
