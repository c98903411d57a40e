"""Frame ingest in front of the TSN extractor: decoded frames or undecoded JPEG files -> uint8 device crops
``[n, 224, 224, C]``, the form the network's first kernel reads.  What the reference does per snippet on the host --
``cv2.imread`` (calcSig_wOF.py:92,105-106) and, inside ``predict_single_frame`` / ``predict_single_flow_stack(...,
frame_size=(340, 256))`` (:94,111), ``cv2.resize`` + crop 0 of the 10-crop over-sample -- runs on the GPU for whole batches.
``oversample_from_*`` cut all ten crops there (``[n * 10, 224, 224, C]``, snippet-major: what the class scores of the TSN test protocol
are averaged over).

A :class:`FrameIngest` depends on the stream's channel count, the device and the resize rule only -- not on any weights -- so the
command line creates it before (and prepares batches while) the extractors are being built, keeps preparing the next stream's
first batches while the current stream's last ones are in the network, and feeds several ensemble members from one decode.
"""
from __future__ import annotations

import atexit
import os
import threading

import numpy as np

from . import frames


# Decoders of closed FrameIngest objects, per device: a decoder's buffers (pinned host memory for the unstuffed streams / coefficients,
# device planes and pixels: 1-2 GB at the command line's batch sizes) cost 40 ms to free and as much to allocate again, so a process that
# runs the command line's main() again (the bench, a broker's worker) takes its decoders from here.  At most _POOL_KEEP idle ones per device.
_POOL_KEEP = 4
_idle_decoders = {}
_idle_lock = threading.Lock()


def _take_decoder(device, h, w):
    with _idle_lock:
        idle = _idle_decoders.get(device, [])
        for k, dec in enumerate(idle):
            if dec.max_h >= h and dec.max_w >= w:
                return idle.pop(k)
    return None


def _give_decoder(device, dec):
    with _idle_lock:
        idle = _idle_decoders.setdefault(device, [])
        if len(idle) < _POOL_KEEP:
            idle.append(dec)
            return
    dec.close()


def drain_decoder_pool():
    """Close the idle decoders (also at interpreter exit)."""
    with _idle_lock:
        idle = [d for ds in _idle_decoders.values() for d in ds]
        _idle_decoders.clear()
    for dec in idle:
        dec.close()


atexit.register(drain_decoder_pool)


def _plane_major(files, i, m, ch):
    """The files of snippets i .. i + m of a flow stream (stack order per snippet), all frames of plane 0 first, then plane 1, ..."""
    return [f for k in range(ch) for f in files[i * ch + k:(i + m) * ch:ch]]


class FrameIngest:
    def __init__(self, channels: int, device: int = 0, resize_rule: str = "cv2"):
        if resize_rule not in frames.RESIZE_RULES:
            raise ValueError("resize_rule must be 'cv2' or 'exact'")
        self._channels, self.device, self._resize_rule = int(channels), int(device), resize_rule
        self._lanes = {}

    def crops_from_frames(self, frames_: np.ndarray, frame_size=(340, 256), crop=224):
        """Decoded frames -> device crops (torch uint8 [n, crop, crop, C]) through vq_resize_crop: RGB frames
        [n, H, W, 3], or flow planes [n, C, H, W] (grey x/y frames in stack order).  Same bytes as frames.crop0."""
        return self._from_frames(frames_, frame_size, crop, ten=False)

    def oversample_from_frames(self, frames_: np.ndarray, frame_size=(340, 256), crop=224):
        """Decoded frames -> the ten over-sampled crops of every snippet on the device (torch uint8 [n * 10, crop, crop, C], row
        10 * i + k = crop k of snippet i): the frames are uploaded once (a tenth of the crops' bytes) and cut by vq_resize_crop with
        VQ_RESIZE_OVERSAMPLE.  RGB frames [n, H, W, 3]: one call; flow planes [n, C, H, W]: a call per plane, the x planes (even) with
        VQ_RESIZE_MIRROR_INVERT.  Same bytes as frames.oversample / frames.oversample_flow_stack."""
        return self._from_frames(frames_, frame_size, crop, ten=True)

    def _rule(self, ten: bool, plane=None):
        """The ``rule`` argument of the resize calls: the ten-crop cut is a flag bit, and so is 255 - v in the mirrors of an x plane (even)
        that goes through vq_resize_crop on its own."""
        rule = frames.RESIZE_RULES[self._resize_rule]
        if ten:
            rule |= frames.RESIZE_OVERSAMPLE | (frames.RESIZE_MIRROR_INVERT if plane is not None and plane % 2 == 0 else 0)
        return rule

    def _resize_crop(self, ptr, on_device, n, h, w, frame_size, crop, ten, dst, stream, plane=None):
        """vq_resize_crop on n packed frames (``plane`` None: all channels) or on grey plane ``plane`` of n stacks -> dst (a pointer)."""
        import ctypes as C
        from .._lib import call
        call("vq_resize_crop", C.c_void_p(ptr), on_device, n, h, w, self._channels if plane is None else 1, frame_size[0], frame_size[1], crop,
             self._rule(ten, plane), C.c_void_p(dst), self._channels, plane or 0, self.device, C.c_void_p(stream))

    def _from_frames(self, frames_, frame_size, crop, ten):
        from . import devmem
        f = np.ascontiguousarray(frames_, dtype=np.uint8)
        if f.ndim != 4:
            raise ValueError("frames must be [n,H,W,3] (RGB) or [n,C,H,W] (flow planes)")
        n = f.shape[0]
        out = devmem.empty_u8((n * 10 if ten else n, crop, crop, self._channels), self.device)
        stream = devmem.current_stream_handle(self.device)
        if self._channels == 3:
            if f.shape[3] != 3:
                raise ValueError("RGB frames must be [n,H,W,3]")
            self._resize_crop(f.ctypes.data, 0, n, f.shape[1], f.shape[2], frame_size, crop, ten, out.data_ptr(), stream)
        else:
            if f.shape[1] != self._channels:
                raise ValueError("flow planes must be [n,%d,H,W]" % self._channels)
            for k in range(self._channels):
                plane = np.ascontiguousarray(f[:, k])
                self._resize_crop(plane.ctypes.data, 0, n, f.shape[2], f.shape[3], frame_size, crop, ten, out.data_ptr(), stream, k)
        return out

    def sync(self):
        """Wait for the resize / crop work of ``crops_from_frames`` (queued on torch's current stream) before an extractor's own
        stream reads the crops."""
        from . import devmem
        devmem.synchronize_current(self.device)

    def crops_from_jpegs(self, files, frame_size=(340, 256), crop=224, lane=0):
        """JPEG file contents -> device crops (torch uint8 [n, crop, crop, C]) without the frames ever visiting the host:
        entropy decoding on the library's host threads, IDCT / upsampling / colour on the device (tsn/jpeg.py), resize +
        crop 0 straight from the decoder's device buffer.  RGB net: n files; flow net: n * C files in stack order per
        snippet (x0, y0, x1, y1, ...).  The pixels are libjpeg's (what cv2.imread returns), bit for bit.  ``lane``: calls of
        different lanes own different decoders and streams and may run at the same time in different threads (the command line
        keeps two batches in preparation: one's host half -- reading, unstuffing -- overlaps the other's device half)."""
        return self._from_jpegs(files, frame_size, crop, lane, ten=False)

    def oversample_from_jpegs(self, files, frame_size=(340, 256), crop=224, lane=0):
        """JPEG files -> the ten over-sampled crops of every snippet on the device (torch uint8 [n * 10, crop, crop, C], snippet-major):
        ``crops_from_jpegs``' decode (same file order, lanes, streams and decoder buffers), then the over-sample cut straight from the
        decoder's device buffer -- the packed call for RGB, the one-launch planes form for the ten planes of a flow stack with an even
        crop, a call per plane otherwise.  Frames that already have ``frame_size`` are copied by the same kernels.  Same bytes as
        decoding on the host + frames.oversample / frames.oversample_flow_stack."""
        return self._from_jpegs(files, frame_size, crop, lane, ten=True)

    def _lane_decoder(self, st, files):
        """A lane's stream and a decoder that holds the frames of ``files`` -> (stream, decoder, files per decoder call, h, w)."""
        from . import devmem, jpeg
        # a stream of its own (non-blocking): the call may run in a thread of its own for a LATER batch while the network works on the
        # current one on the default stream -- decoding a batch of flow files keeps a few CUs busy for tens of milliseconds
        if st["stream"] is None:
            # (a high-priority stream was tried for the decode kernels in round 4: no gain, 385-391 against 394-412 clips/s end to end.
            # Round 6, VQ_INGEST_PRIORITY=low|normal|high on one box: 576 / 576 / 577 and 575 / 531 / 571 clips/s -- the queue priority of the
            # ingest kernels does not change what the networks get; the default stays normal.)
            prio = {"low": -1, "normal": 0, "high": 1}.get(os.environ.get("VQ_INGEST_PRIORITY", "normal"), 0)
            st["stream"] = devmem.new_stream(self.device, prio)
        ingest = st["stream"]
        h, w, _ = jpeg.info(files[0])
        # files per decoder call (its buffers grow to what a call needs; a call addresses its component planes with 32 bits)
        cap = max(1, min(8192, int(3.0e9 // (2 * (h + 16) * (w + 16)))))
        dec = st["jpeg"]
        if dec is None or dec.max_h < h or dec.max_w < w:
            if dec is not None:
                dec.close()
            dec = st["jpeg"] = _take_decoder(self.device, h, w) or jpeg.JpegDecoder(cap, h, w, self.device)
        return ingest, dec, min(cap, dec.max_frames), h, w

    def _from_jpegs(self, files, frame_size, crop, lane, ten):
        import ctypes as C
        from .._lib import call
        from . import devmem
        ch = self._channels
        per_snip = 1 if ch == 3 else ch
        if len(files) % per_snip:
            raise ValueError("flow net: %d files is not a multiple of the %d planes of a snippet" % (len(files), ch))
        n = len(files) // per_snip
        rows = 10 if ten else 1                          # crops per snippet
        out = devmem.empty_u8((n * rows, crop, crop, ch), self.device)
        st = self._lanes.setdefault(lane, {"stream": None, "jpeg": None, "lock": threading.Lock()})
        with st["lock"]:                                 # a lane's decoder buffer and stream serve one call at a time
            ingest, dec, cap, h, w = self._lane_decoder(st, files)
            stream = ingest.cuda_stream
            same_size = (w, h) == tuple(frame_size) and crop % 2 == 0 and crop <= min(h, w)
            # frames as build_wof_clips.py writes them: resize is the identity, crop 0 the top-left pixels -- decoded and cropped without the
            # whole-frame pixel pass in between (8 000 grey frames per flow batch: 0.7 GB written and read again for the 57 % that survive)
            direct = not ten and same_size and ch in (3, 10)
            # the grey frames of `per` snippets in ONE decoder call, plane-major (all x0 frames, then all y0 frames, ...): a batch of
            # 32 clips x 25 snippets is 8 000 small files -- the size at which the entropy decoding runs on the device -- and every
            # plane's frames are contiguous for the resize that interleaves them into the 10-channel crops
            per = cap if ch == 3 else max(1, cap // ch)
            for i in range(0, n, per):
                m = min(per, n - i)
                group = files[i:i + m] if ch == 3 else _plane_major(files, i, m, ch)
                dst = out[rows * i:rows * (i + m)].data_ptr()
                if direct:
                    dec.decode_to_crops(group, ch == 3, crop, dst, planes=ch, stream=stream)
                    continue
                ptr, _ = dec.decode_to_device(group, color=ch == 3, stream=stream)
                if ch == 3:
                    self._resize_crop(ptr, 1, m, h, w, frame_size, crop, ten, dst, stream)
                elif ch == 10 and crop % 2 == 0:
                    # the ten planes of the stacks in ONE launch (taps once per pixel, whole-word stores; frames that have the size already
                    # are copied): 10 launches of 0.53 ms per 800 crops took 5.3 ms of the GPU per batch beside the networks
                    call("vq_resize_crop_planes", C.c_void_p(ptr), m, h, w, ch, m * h * w, frame_size[0], frame_size[1], crop, self._rule(ten),
                         C.c_void_p(dst), self.device, C.c_void_p(stream))
                else:
                    for k in range(ch):
                        self._resize_crop(ptr + k * m * h * w, 1, m, h, w, frame_size, crop, ten, dst, stream, k)
                ingest.synchronize()                                  # the decoder's buffer is reused by its next call
        return out

    def close(self):
        for st in self._lanes.values():
            if st["jpeg"] is not None:
                _give_decoder(self.device, st["jpeg"])             # idle, not freed: see _idle_decoders
                st["jpeg"] = None
