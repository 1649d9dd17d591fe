"""Host-side mirror of psyne's TDT protocol over the gfx950 codec (libpsyne_tdt.so).

Reference interface (include/psyne/protocol/tdt_compression.hpp):
  TDTConfig                 :31-43
  TDTCompressionProtocol    :176-638 — should_transform, analyze_data, encode, decode,
                            update_network_metrics, update_system_metrics, protocol_name,
                            is_lossless, transformation_ratio, processing_overhead_ms,
                            get_average_entropy, get_bandwidth_mbps, get_cpu_usage
satisfying psyne::concepts::Protocol (include/psyne/concepts/protocol_concepts.hpp:22-47).

Two layers:
  * ``TdtCodec`` — the batch API: device-resident torch.uint8 tensors of concatenated
    messages plus int64 offsets (n+1), asynchronous on the current torch stream.  This is
    the hot path (bench.py measures it).
  * ``TDTCompressionProtocol`` — the reference's one-message-per-call API (host bytes in,
    host bytes out) with the same names, defaults, exceptions and metric semantics, built
    on the C ABI's host path.

torch is used only for device memory and streams; all codec work is in the HIP kernels.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import time
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import TdtConfigC, TdtError, check

MAGIC_TDT = 0x54445444
MAGIC_UNCP = 0x554E4350


@dataclass
class TDTConfig:
    """TDTConfig (tdt_compression.hpp:31-43).  auto_detect_clusters / max_clusters /
    enable_simd are declared by the reference but never read; kept for API parity.
    sample_fraction is accepted, but the GPU always analyses every word (the reference's
    sample_fraction = 1.0 behaviour, which is the only deterministic one).  word_size: any record
    stride in 1..64 (1, 2, 4, 8, 16 on the tuned kernels, the others on the generic ones)."""
    sample_fraction: float = 0.3
    word_size: int = 4
    auto_detect_clusters: bool = True
    max_clusters: int = 4
    enable_simd: bool = True
    bandwidth_threshold_mbps: float = 100.0
    cpu_usage_threshold: float = 0.8
    min_tensor_size: int = 1024

    def to_c(self) -> TdtConfigC:
        return TdtConfigC(self.sample_fraction, self.word_size, self.bandwidth_threshold_mbps,
                          self.cpu_usage_threshold, self.min_tensor_size)


def transformation_ratio_of(blob: bytes, n: int) -> float | None:
    """The reference's transformation_ratio() after encoding n bytes into `blob`
    (compress_tdt :395-396): n / TDTEncodedData::encoded_size() (:71-78), which counts the RLE
    stream bytes, the mapping ints and sizeof(TDTEncodedData) = 72 (x86-64 libstdc++: two
    vectors, size_t, int, double) — not the serialized length.  None for a UNCP blob (the
    reference leaves the ratio unchanged on the passthrough path, :230-236 and :256-265)."""
    if len(blob) < 20 or int.from_bytes(blob[:4], "little") != MAGIC_TDT:
        return None
    ns = int.from_bytes(blob[8:12], "little")
    msize = int.from_bytes(blob[16:20], "little")
    streams = len(blob) - 20 - 4 * msize - 4 * ns
    return float(n) / float(streams + 4 * msize + 72)


def encode_bound(n: int, word_size: int = 4) -> int:
    return int(_lib.load().tdt_encode_bound(n, word_size))


def mapbits_of(mapping) -> int:
    """The mapping bits (one word per message: mappings_v, the mapbits= arguments) of a mapping given
    as one stream number in {0, 1} per byte position: bit p = mapping[p]."""
    mapping = [int(m) for m in mapping]
    if not 1 <= len(mapping) <= 64:
        raise ValueError("a mapping holds 1..64 positions")
    bits = 0
    for p, m in enumerate(mapping):
        if m not in (0, 1):
            raise ValueError("mapping[%d] = %d is neither 0 nor 1" % (p, m))
        bits |= m << p
    return bits


def mapping_of(bits: int, ws: int) -> list[int]:
    """The mapping (one stream number per byte position, as blobs carry it at bytes 20 ..) of mapping
    bits at word size ws; a bit at or above ws is TDT_E_BAD_MAPPING's case and raises here."""
    bits = int(bits) & 0xFFFFFFFFFFFFFFFF  # (an int64 tensor's entry with bit 63 set reads negative)
    if not 1 <= ws <= 64:
        raise ValueError("word size %d is outside 1..64" % ws)
    if bits >> ws:
        raise ValueError("mapping bits 0x%x have a bit at or above word size %d" % (bits, ws))
    return [(bits >> p) & 1 for p in range(ws)]


def _ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


class TdtCodec:
    """Batched TDT codec bound to one HIP device."""

    def __init__(self, config: TDTConfig | None = None, device: int = 0, lib=None, raw_fallback: bool = False,
                 host_raw_fallback: bool = False):
        """raw_fallback=True sets TDT_OPT_RAW_FALLBACK: the batch encodes store a message whose TDT blob
        would be longer than the message plus 4 bytes as its UNCP blob (marker + the raw bytes), so a blob
        never exceeds n + 4 bytes, and the bounds, slots and allocations below follow.
        host_raw_fallback=True sets TDT_OPT_HOST_RAW_FALLBACK: the same rule for encode_host (the host
        pipeline and its one-message path), whose bound is host_encode_bound.  The two are independent."""
        self.config = config or TDTConfig()
        self.device = device
        self._lib = lib if lib is not None else _lib.load()  # `lib`: diagnostic builds only
        h = C.c_void_p()
        cfg = self.config.to_c()
        check(self._lib.tdt_ctx_create(device, C.byref(cfg), C.byref(h)))
        self._h = h
        if raw_fallback:
            self.set_option(_lib.TDT_OPT_RAW_FALLBACK, 1)
        if host_raw_fallback:
            self.set_option(_lib.TDT_OPT_HOST_RAW_FALLBACK, 1)

    @property
    def host_raw_fallback(self) -> bool:
        """Whether the context runs with TDT_OPT_HOST_RAW_FALLBACK, however it was set (asked of the
        context, as raw_fallback is)."""
        return self.host_encode_bound(0) == 4

    def host_encode_bound(self, n: int) -> int:
        """tdt_ctx_host_encode_bound: what encode_host may write for an n-byte message — n + 4 under
        host_raw_fallback, else the TDT bound at this codec's word_size."""
        f = getattr(self._lib, "tdt_ctx_host_encode_bound", None)
        if f is None:  # (an older build chosen for an A/B run, which has no host raw fallback either)
            return int(self._lib.tdt_encode_bound(n, self.config.word_size))
        return int(f(self._h, n))

    @property
    def raw_fallback(self) -> bool:
        """Whether the context runs with TDT_OPT_RAW_FALLBACK — however it was set: the constructor,
        set_option or PSYNE_TDT_RAW_FALLBACK.  Asked of the context: its bound of a message is n + 4
        exactly then (the TDT bound is at least 2n + 32)."""
        return self.encode_bound(0) == 4

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tdt_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- policy (update_network_metrics / update_system_metrics :309-319)
    def set_metrics(self, bandwidth_mbps: float, latency_ms: float = 1.0, cpu_usage: float = 0.5):
        self._lib.tdt_ctx_set_metrics(self._h, bandwidth_mbps, latency_ms, cpu_usage)

    def get_metrics(self) -> tuple[float, float, float]:
        b, l, c = C.c_double(), C.c_double(), C.c_double()
        self._lib.tdt_ctx_get_metrics(self._h, C.byref(b), C.byref(l), C.byref(c))
        return b.value, l.value, c.value

    def set_size_hint(self, typical_message_bytes: int):
        self._lib.tdt_ctx_set_size_hint(self._h, typical_message_bytes)

    def should_transform(self, n: int) -> bool:
        return bool(self._lib.tdt_should_transform(self._h, n))

    def encode_bound(self, n: int) -> int:
        """tdt_ctx_encode_bound: n + 4 under raw_fallback, else the TDT bound at this codec's word_size."""
        f = getattr(self._lib, "tdt_ctx_encode_bound", None)
        if f is None:  # (an older build chosen for an A/B run, which has no raw fallback either)
            return int(self._lib.tdt_encode_bound(n, self.config.word_size))
        return int(f(self._h, n))

    @staticmethod
    def _tdt_bounds(sizes, ws):
        """tdt_encode_bound over a host int64 array of sizes at width(s) `ws`: what the calls that ignore
        TDT_OPT_RAW_FALLBACK (the host calls, encode_batch(mapping=...)) may write."""
        return np.maximum(sizes + 4, 28 + 4 * ws + 2 * sizes)

    def _bounds(self, sizes, ws):
        """tdt_ctx_encode_bound over a host int64 array of sizes at width(s) `ws`."""
        return sizes + 4 if self.raw_fallback else self._tdt_bounds(sizes, ws)

    # ---- batches (device tensors) ------------------------------------------------------
    @staticmethod
    def _stream(stream):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return C.c_void_p(s.cuda_stream)

    def batch_bound(self, offsets_host: np.ndarray) -> int:
        sizes = np.diff(np.asarray(offsets_host, dtype=np.int64))
        return int(self._bounds(sizes, self.config.word_size).sum()) if sizes.size else 0

    def encode_batch(self, data, offsets, out=None, out_offsets=None, status=None, mapping=None,
                     out_capacity: int | None = None, stream=None):
        """Encode messages data[offsets[i]:offsets[i+1]] (torch uint8 / int64 on the GPU).
        Returns (out, out_offsets, status); blobs are compacted in message order."""
        import torch
        n = offsets.numel() - 1
        if out is None:
            cap = out_capacity
            if cap is None and mapping is not None:  # (tdt_encode_with_mapping_batch ignores TDT_OPT_RAW_FALLBACK)
                cap = int(self._tdt_bounds(np.diff(offsets.cpu().numpy().astype(np.int64)), self.config.word_size).sum())
            elif cap is None:
                cap = self.batch_bound(offsets.cpu().numpy())
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=data.device)
        if out_offsets is None:
            out_offsets = torch.empty(n + 1, dtype=torch.int64, device=data.device)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.int32, device=data.device)
        cap = out.numel() if out_capacity is None else out_capacity
        if mapping is None:
            check(self._lib.tdt_encode_batch(self._h, _ptr(data), _ptr(offsets), n, _ptr(out), cap,
                                             _ptr(out_offsets), _ptr(status), self._stream(stream)))
        else:
            check(self._lib.tdt_encode_with_mapping_batch(self._h, _ptr(data), _ptr(offsets), n, _ptr(mapping),
                                                          _ptr(out), cap, _ptr(out_offsets), _ptr(status),
                                                          self._stream(stream)))
        return out, out_offsets, status

    def decode_batch(self, blobs, offsets, out=None, out_offsets=None, status=None,
                     out_capacity: int | None = None, stream=None):
        """Decode blobs[offsets[i]:offsets[i+1]].  If `out` is None the decoded sizes are
        computed first (tdt_decoded_sizes_batch) to size it."""
        import torch
        n = offsets.numel() - 1
        if out is None:
            sizes, _ = self.decoded_sizes(blobs, offsets, stream=stream)
            cap = int(sizes.sum().item())
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=blobs.device)
        if out_offsets is None:
            out_offsets = torch.empty(n + 1, dtype=torch.int64, device=blobs.device)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.int32, device=blobs.device)
        cap = out.numel() if out_capacity is None else out_capacity
        check(self._lib.tdt_decode_batch(self._h, _ptr(blobs), _ptr(offsets), n, _ptr(out), cap,
                                         _ptr(out_offsets), _ptr(status), self._stream(stream)))
        return out, out_offsets, status

    # ---- slotted batches (no inter-message dependency: the hot path) -------------------
    def encode_slots(self, offsets, stream=None):
        """Slot offsets (n+1, int64, device) = prefix sum of the encode bounds."""
        import torch
        n = offsets.numel() - 1
        slots = torch.empty(n + 1, dtype=torch.int64, device=offsets.device)
        check(self._lib.tdt_encode_slots(self._h, _ptr(offsets), n, _ptr(slots), self._stream(stream)))
        return slots

    def decode_slots(self, blobs, offsets, lengths=None, status=None, stream=None):
        """Slot offsets (n+1) = prefix sum of the decoded sizes (header parse).  With
        `lengths`, blob i is blobs[offsets[i]:offsets[i]+lengths[i]] (offsets may then have n
        or n+1 entries)."""
        import torch
        n = lengths.numel() if lengths is not None else offsets.numel() - 1
        slots = torch.empty(n + 1, dtype=torch.int64, device=offsets.device)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.int32, device=offsets.device)
        check(self._lib.tdt_decode_slots(self._h, _ptr(blobs), _ptr(offsets), _ptr(lengths), n, _ptr(slots),
                                         _ptr(status), self._stream(stream)))
        return slots

    def encode_into(self, data, offsets, slots=None, out=None, lengths=None, status=None, stream=None):
        """Encode message i into out[slots[i]:slots[i+1]]; returns (out, slots, lengths, status)."""
        import torch
        n = offsets.numel() - 1
        if slots is None:
            slots = self.encode_slots(offsets, stream=stream)
        if out is None:
            out = torch.empty(max(int(slots[-1].item()), 1), dtype=torch.uint8, device=data.device)
        if lengths is None:
            lengths = torch.empty(max(n, 1), dtype=torch.int64, device=data.device)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.int32, device=data.device)
        check(self._lib.tdt_encode_batch_into(self._h, _ptr(data), _ptr(offsets), n, _ptr(out), _ptr(slots),
                                              _ptr(lengths), _ptr(status), self._stream(stream)))
        return out, slots, lengths, status

    def decode_into(self, blobs, offsets, in_lengths=None, slots=None, out=None, lengths=None, status=None,
                    stream=None):
        """Decode blob i (blobs[offsets[i]:offsets[i]+in_lengths[i]], or up to offsets[i+1]) into
        out[slots[i]:slots[i+1]]; returns (out, slots, lengths, status)."""
        import torch
        n = in_lengths.numel() if in_lengths is not None else offsets.numel() - 1
        if slots is None:
            slots = self.decode_slots(blobs, offsets, lengths=in_lengths, stream=stream)
        if out is None:
            out = torch.empty(max(int(slots[-1].item()), 1), dtype=torch.uint8, device=blobs.device)
        if lengths is None:
            lengths = torch.empty(max(n, 1), dtype=torch.int64, device=blobs.device)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.int32, device=blobs.device)
        check(self._lib.tdt_decode_batch_into(self._h, _ptr(blobs), _ptr(offsets), _ptr(in_lengths), n, _ptr(out),
                                              _ptr(slots), _ptr(lengths), _ptr(status), self._stream(stream)))
        return out, slots, lengths, status

    def decoded_sizes(self, blobs, offsets, stream=None):
        import torch
        n = offsets.numel() - 1
        sizes = torch.empty(max(n, 1), dtype=torch.int64, device=blobs.device)
        status = torch.empty(max(n, 1), dtype=torch.int32, device=blobs.device)
        check(self._lib.tdt_decoded_sizes_batch(self._h, _ptr(blobs), _ptr(offsets), n, _ptr(sizes),
                                                _ptr(status), self._stream(stream)))
        return sizes[:n], status[:n]

    # ---- scattered batches (one buffer per message: tensors of a training process) ------
    @staticmethod
    def _check_mapbits(mapbits, n):
        import torch
        if mapbits.dtype != torch.int64 or mapbits.numel() < n:
            raise ValueError("mapbits must be an int64 tensor of one word per message")

    def encode_v(self, ptrs, sizes, out_ptrs, out_caps, lengths=None, status=None, stream=None, mapbits=None):
        """Encode message i = sizes[i] bytes at address ptrs[i] into out_caps[i] bytes at address
        out_ptrs[i] (int64 tensors on the GPU); returns (lengths, status).  mapbits (an int64 tensor on
        the GPU, one word per message: mappings_v's, or mapbits_of) encodes with those mappings instead
        of analysing the messages; a word with a bit at or above the word size gives status 4."""
        import torch
        n = sizes.numel()
        if lengths is None:
            lengths = torch.empty(max(n, 1), dtype=torch.int64, device=sizes.device)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.int32, device=sizes.device)
        if mapbits is not None:
            self._check_mapbits(mapbits, n)
            check(self._lib.tdt_encode_mapped_v(self._h, _ptr(ptrs), _ptr(sizes), None, 0, n, _ptr(mapbits),
                                                _ptr(out_ptrs), _ptr(out_caps), _ptr(lengths), _ptr(status),
                                                self._stream(stream)))
            return lengths, status
        check(self._lib.tdt_encode_batch_v(self._h, _ptr(ptrs), _ptr(sizes), n, _ptr(out_ptrs), _ptr(out_caps),
                                           _ptr(lengths), _ptr(status), self._stream(stream)))
        return lengths, status

    @staticmethod
    def width_mask(word_sizes) -> int:
        """The mask encode_vw takes: bit w - 1 set for every width w in `word_sizes` (host ints)."""
        mask = 0
        for w in set(int(w) for w in word_sizes):
            if not 1 <= w <= 64:
                raise ValueError("word size %d is outside 1..64" % w)
            mask |= 1 << (w - 1)
        return mask

    def encode_vw(self, ptrs, sizes, word_sizes, width_mask, out_ptrs, out_caps, lengths=None, status=None,
                  stream=None, mapbits=None):
        """encode_v with one record width per message: word_sizes[i] (int32 tensor on the GPU) is
        message i's, whatever this codec's own word_size; width_mask (a host int, bit w - 1 per width
        that may occur, at most 8 of them) tells the host which pipelines to launch.  Blob i is what
        a codec of word_size word_sizes[i] gives; returns (lengths, status).  mapbits: as for encode_v."""
        import torch
        n = sizes.numel()
        if n and word_sizes.dtype != torch.int32:
            raise ValueError("word_sizes must be an int32 tensor")
        if lengths is None:
            lengths = torch.empty(max(n, 1), dtype=torch.int64, device=sizes.device)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.int32, device=sizes.device)
        if mapbits is not None:
            self._check_mapbits(mapbits, n)
            check(self._lib.tdt_encode_mapped_v(self._h, _ptr(ptrs), _ptr(sizes), _ptr(word_sizes), int(width_mask), n,
                                                _ptr(mapbits), _ptr(out_ptrs), _ptr(out_caps), _ptr(lengths),
                                                _ptr(status), self._stream(stream)))
            return lengths, status
        check(self._lib.tdt_encode_batch_vw(self._h, _ptr(ptrs), _ptr(sizes), _ptr(word_sizes), int(width_mask), n,
                                            _ptr(out_ptrs), _ptr(out_caps), _ptr(lengths), _ptr(status),
                                            self._stream(stream)))
        return lengths, status

    def decode_v(self, ptrs, in_lengths, out_ptrs, out_caps, lengths=None, status=None, stream=None):
        """Decode blob i = in_lengths[i] bytes at address ptrs[i] into out_caps[i] bytes at address
        out_ptrs[i] (int64 tensors on the GPU); returns (lengths, status)."""
        import torch
        n = in_lengths.numel()
        if lengths is None:
            lengths = torch.empty(max(n, 1), dtype=torch.int64, device=in_lengths.device)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.int32, device=in_lengths.device)
        check(self._lib.tdt_decode_batch_v(self._h, _ptr(ptrs), _ptr(in_lengths), n, _ptr(out_ptrs), _ptr(out_caps),
                                           _ptr(lengths), _ptr(status), self._stream(stream)))
        return lengths, status

    def decoded_sizes_v(self, ptrs, in_lengths, stream=None):
        import torch
        n = in_lengths.numel()
        sizes = torch.empty(max(n, 1), dtype=torch.int64, device=in_lengths.device)
        status = torch.empty(max(n, 1), dtype=torch.int32, device=in_lengths.device)
        check(self._lib.tdt_decoded_sizes_v(self._h, _ptr(ptrs), _ptr(in_lengths), n, _ptr(sizes), _ptr(status),
                                            self._stream(stream)))
        return sizes[:n], status[:n]

    # ---- exact encoded sizes (how long blob i will be, before it is written) -----------------
    def encoded_sizes(self, data, offsets, stream=None, enc_sizes=None, status=None):
        """The exact length of the blob of message i = data[offsets[i]:offsets[i+1]] at this codec's
        word_size, without encoding it: (sizes, status), int64 / int32 tensors on the GPU.  sizes[i]
        is what encode_v reports for a capacity of the encode bound, and sizes[i] / message size the
        message's transformation ratio.  enc_sizes / status: the caller's result tensors (n entries;
        pass them when the call is captured into a graph, so that nothing is allocated in the capture
        and every replay writes where the caller reads)."""
        import torch
        n = offsets.numel() - 1
        sizes = enc_sizes if enc_sizes is not None else torch.empty(max(n, 1), dtype=torch.int64, device=offsets.device)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.int32, device=offsets.device)
        check(self._lib.tdt_encoded_sizes_batch(self._h, _ptr(data), _ptr(offsets), n, _ptr(sizes), _ptr(status),
                                                self._stream(stream)))
        return sizes[:n], status[:n]

    def encoded_sizes_v(self, ptrs, sizes, word_sizes=None, width_mask=0, stream=None, enc_sizes=None, status=None):
        """encoded_sizes for scattered messages (sizes[i] bytes at address ptrs[i], int64 tensors on the
        GPU): at this codec's word_size (word_sizes None), or at word_sizes[i] per message with
        width_mask as encode_vw takes them — a rejected width gets its status and size 0.  Returns
        (enc_sizes, status); enc_sizes / status may be the caller's tensors, as for encoded_sizes."""
        import torch
        n = sizes.numel()
        if n and word_sizes is not None and word_sizes.dtype != torch.int32:
            raise ValueError("word_sizes must be an int32 tensor")
        enc = enc_sizes if enc_sizes is not None else torch.empty(max(n, 1), dtype=torch.int64, device=sizes.device)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.int32, device=sizes.device)
        check(self._lib.tdt_encoded_sizes_v(self._h, _ptr(ptrs), _ptr(sizes), _ptr(word_sizes), int(width_mask), n,
                                            _ptr(enc), _ptr(status), self._stream(stream)))
        return enc[:n], status[:n]

    def mappings_v(self, ptrs, sizes, word_sizes=None, width_mask=0, stream=None, enc_sizes=None, mapbits=None,
                   status=None):
        """encoded_sizes_v plus the mapping the encode decides for every message: (enc_sizes, mapbits,
        status), mapbits an int64 tensor of one word per message (bit p = the stream of byte position
        p; 0 for a message that goes through uncompressed or whose width is rejected).  Passed back as
        encode_v / encode_vw / encode_vp / encode_tensors(mapbits=...) it gives the bytes of the
        ordinary encode without the analysis: size and map every K steps, encode mapped between."""
        import torch
        n = sizes.numel()
        if n and word_sizes is not None and word_sizes.dtype != torch.int32:
            raise ValueError("word_sizes must be an int32 tensor")
        enc = enc_sizes if enc_sizes is not None else torch.empty(max(n, 1), dtype=torch.int64, device=sizes.device)
        bits = mapbits if mapbits is not None else torch.empty(max(n, 1), dtype=torch.int64, device=sizes.device)
        self._check_mapbits(bits, n)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.int32, device=sizes.device)
        check(self._lib.tdt_mappings_v(self._h, _ptr(ptrs), _ptr(sizes), _ptr(word_sizes), int(width_mask), n,
                                       _ptr(enc), _ptr(bits), _ptr(status), self._stream(stream)))
        return enc[:n], bits[:n], status[:n]

    # ---- packed wire buffer (blobs back to back, one copy or send per batch) ----------------
    def pack_v(self, ptrs, lengths, out, out_offsets=None, status=None, stream=None):
        """Pack blob i = lengths[i] bytes at address ptrs[i] (int64 tensors on the GPU: the slots and
        lengths of encode_into, or the blobs of encode_v / encode_vw) into out[offsets[i]:offsets[i+1]],
        offsets (n + 1, int64, device) being the prefix sum of the lengths.  A blob that ends past
        out.numel() gets status 5 (TDT_E_CAPACITY) and is not copied; offsets[n] is the full need
        either way.  Returns (out_offsets, status)."""
        import torch
        n = lengths.numel()
        if out_offsets is None:
            out_offsets = torch.zeros(n + 1, dtype=torch.int64, device=lengths.device)
        if status is None:
            status = torch.zeros(max(n, 1), dtype=torch.int32, device=lengths.device)
        check(self._lib.tdt_pack_v(self._h, _ptr(ptrs), _ptr(lengths), n, _ptr(out), out.numel(), _ptr(out_offsets),
                                   _ptr(status), self._stream(stream)))
        return out_offsets, status

    def encode_vp(self, ptrs, sizes, total_bytes, out, word_sizes=None, width_mask=0, out_offsets=None, status=None,
                  stream=None, mapbits=None):
        """encode_v (word_sizes None) or encode_vw (word_sizes an int32 tensor on the GPU, width_mask
        as there) into the packed buffer `out`: blob i at out[offsets[i]:offsets[i+1]].  total_bytes
        (a host int) is an upper bound of sizes.sum(): it sizes the codec's scratch, and the host
        reads nothing back.  A blob that ends past out.numel() gets status 5 (TDT_E_CAPACITY);
        offsets[n] is the full need either way.  Returns (out_offsets, status).  mapbits: as for
        encode_v (the mapped packed call always takes the two phases)."""
        import torch
        n = sizes.numel()
        if n and word_sizes is not None and word_sizes.dtype != torch.int32:
            raise ValueError("word_sizes must be an int32 tensor")
        if out_offsets is None:
            out_offsets = torch.zeros(n + 1, dtype=torch.int64, device=sizes.device)
        if status is None:
            status = torch.zeros(max(n, 1), dtype=torch.int32, device=sizes.device)
        if mapbits is not None:
            self._check_mapbits(mapbits, n)
            check(self._lib.tdt_encode_mapped_vp(self._h, _ptr(ptrs), _ptr(sizes), _ptr(word_sizes), int(width_mask), n,
                                                 int(total_bytes), _ptr(mapbits), _ptr(out), out.numel(),
                                                 _ptr(out_offsets), _ptr(status), self._stream(stream)))
            return out_offsets, status
        check(self._lib.tdt_encode_batch_vp(self._h, _ptr(ptrs), _ptr(sizes), _ptr(word_sizes), int(width_mask), n,
                                            int(total_bytes), _ptr(out), out.numel(), _ptr(out_offsets), _ptr(status),
                                            self._stream(stream)))
        return out_offsets, status

    @staticmethod
    def _tensor_table(tensors):
        """(addresses, byte sizes) of a list of contiguous GPU tensors, as host int64 arrays."""
        for t in tensors:
            if not t.is_cuda:
                raise ValueError("encode_tensors / decode_tensors take GPU tensors")
            if not t.is_contiguous():
                raise ValueError("encode_tensors / decode_tensors take contiguous tensors")
        sizes = np.array([t.numel() * t.element_size() for t in tensors], dtype=np.int64)
        ptrs = np.array([t.data_ptr() if s else 0 for t, s in zip(tensors, sizes)], dtype=np.uint64).view(np.int64)
        return ptrs, sizes

    def encode_tensors(self, tensors, out=None, stream=None, word_sizes=None, packed=False, exact=False, mapbits=None,
                       return_mappings=False):
        """Encode a list of contiguous GPU tensors (message i = the bytes of tensors[i]) without
        packing them: blob i goes to out[slots[i]:slots[i+1]], the slots being the prefix sum of the
        encode bounds.  Returns (out, slots, lengths, status).

        Tensors of any dtypes are accepted; `word_sizes` says at which record width each is encoded:
          None      every tensor at this codec's word_size, whatever its dtype (a bfloat16 tensor at
                    word_size 4 is split on float32's byte planes, and a tensor whose byte size is
                    no multiple of word_size goes through uncompressed);
          "dtype"   tensor i at its element_size() (2 for bfloat16 / float16, 4 for float32, 8 for
                    float64 / int64, 1 for uint8), in one call;
          ints      one width in 1..64 per tensor.
        With widths, at most 8 different ones may occur in a call; blob i is what a codec of that
        word_size gives.  decode_tensors needs no widths: blobs carry theirs.

        packed=True gives the wire form instead: the blobs back to back in `out`, and the return value
        is (out, offsets, status) with offsets holding n + 1 entries on the GPU, so that
        out[:offsets[n]] is what one copy or one send ships.  The round trip:
            out, offsets, status = codec.encode_tensors(tensors, packed=True)
            codec.decode_tensors(out, offsets, offsets[1:] - offsets[:-1], outs)
        `out` defaults to the sum of the encode bounds, as in the slotted form: TDT does not fall back
        to the raw bytes when its run-length streams grow, so a blob of incompressible records reaches
        28 + 4*ws + 2*size and a buffer of the sizes plus a margin would not hold it.  A smaller `out`
        may be passed: a blob that ends past it gets status 5 and offsets[n] still reports the need.

        packed=True, exact=True allocates exactly what the blobs need instead: the tensors are sized
        on the GPU (encoded_sizes_v), the sizes summed there, and the total is read back — ONE
        synchronisation of the stream with the host, which the other forms do not have — then `out`
        is allocated with that many bytes (a caller's `out` is ignored) and every blob is encoded
        straight to its offset.  Returns (out, offsets, status) as packed=True does, with
        out.numel() == offsets[n].

        Known mappings: mapbits (an int64 tensor on the GPU, one word per tensor) encodes every tensor
        with that mapping instead of analysing it; return_mappings=True first decides the mappings
        (mappings_v), encodes with them, and appends the mapping tensor to the returned tuple — keep
        it and pass it as mapbits for the following steps:
            out, slots, lengths, status, bits = codec.encode_tensors(grads, return_mappings=True)
            out, slots, lengths, status = codec.encode_tensors(grads, mapbits=bits)   # steps 2 .. K
        (exact=True sizes the blobs under the mappings the codec decides, so with it mapbits must be
        those of the same bytes, as return_mappings=True makes them: a stale mapping's longer blob
        gets status 5 there.)"""
        import torch
        ptrs, sizes = self._tensor_table(tensors)
        n = len(tensors)
        if return_mappings and mapbits is not None:
            raise ValueError("return_mappings=True decides the mappings itself: pass no mapbits")
        if return_mappings:
            res = self._encode_tensors_mapped(tensors, ptrs, sizes, out, stream, word_sizes, packed, exact)
            return res
        if mapbits is not None:
            self._check_mapbits(mapbits, n)
        dev = tensors[0].device if n else torch.device("cuda", self.device)
        if word_sizes is None:
            widths = None
            ws = self.config.word_size
        else:
            if isinstance(word_sizes, str):
                if word_sizes != "dtype":
                    raise ValueError('word_sizes is None, "dtype" or one width per tensor')
                widths = np.array([t.element_size() for t in tensors], dtype=np.int32)
            else:
                widths = np.array([int(w) for w in word_sizes], dtype=np.int32)
            if widths.size != n:
                raise ValueError("%d word sizes for %d tensors" % (widths.size, n))
            mask = self.width_mask(widths)
            if bin(mask).count("1") > 8:
                raise ValueError("more than 8 different word sizes in one call")
            ws = widths.astype(np.int64)
        if exact and not packed:
            raise ValueError("exact=True sizes the packed form: pass packed=True")
        if packed and exact:
            parts = [ptrs, sizes]  # one upload: addresses | sizes (| widths, two per word)
            if widths is not None:
                parts.append(np.concatenate([widths, np.zeros(n % 2, np.int32)]).view(np.int64))
            d = torch.from_numpy(np.concatenate(parts)).to(dev, non_blocking=False)
            dw = d[2 * n:].view(torch.int32)[:n] if widths is not None and n else None
            enc, status = self.encoded_sizes_v(d[:n], d[n:2 * n], word_sizes=dw, width_mask=mask if dw is not None else 0,
                                               stream=stream)
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                torch.cumsum(enc, 0, out=offsets[1:])
                total = int(offsets[n].item()) if n else 0  # (the one read-back)
                out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)[:total]
                optrs = offsets[:n] + out.data_ptr()
                caps = offsets[1:] - offsets[:n]
            if n == 0:
                return out, offsets, status
            if dw is None:
                _, status = self.encode_v(d[:n], d[n:2 * n], optrs, caps, stream=stream, mapbits=mapbits)
            else:
                _, status = self.encode_vw(d[:n], d[n:2 * n], dw, mask, optrs, caps, stream=stream, mapbits=mapbits)
            return out, offsets, status[:n]
        slots = np.zeros(n + 1, np.int64)
        np.cumsum(self._bounds(sizes, ws), out=slots[1:])
        if packed:
            if out is None:
                out = torch.empty(max(int(slots[-1]), 1), dtype=torch.uint8, device=dev)
            parts = [ptrs, sizes]  # one upload: addresses | sizes (| widths, two per word)
            if widths is not None:
                parts.append(np.concatenate([widths, np.zeros(n % 2, np.int32)]).view(np.int64))
            d = torch.from_numpy(np.concatenate(parts)).to(dev, non_blocking=False)
            dw = d[2 * n:].view(torch.int32)[:n] if widths is not None and n else None
            offsets, status = self.encode_vp(d[:n], d[n:2 * n], int(sizes.sum()), out, word_sizes=dw,
                                             width_mask=mask if dw is not None else 0, stream=stream, mapbits=mapbits)
            return out, offsets, status
        if out is None:
            out = torch.empty(max(int(slots[-1]), 1), dtype=torch.uint8, device=dev)
        elif out.numel() < int(slots[-1]):
            raise ValueError("out holds %d bytes, the slots need %d" % (out.numel(), int(slots[-1])))
        # one upload: addresses | sizes | blob addresses | capacities | slots (| widths, two per word)
        parts = [ptrs, sizes, out.data_ptr() + slots[:-1], np.diff(slots), slots]
        if widths is not None:
            parts.append(np.concatenate([widths, np.zeros(n % 2, np.int32)]).view(np.int64))
        d = torch.from_numpy(np.concatenate(parts)).to(dev, non_blocking=False)
        if widths is None or n == 0:
            lengths, status = self.encode_v(d[:n], d[n:2 * n], d[2 * n:3 * n], d[3 * n:4 * n], stream=stream,
                                            mapbits=mapbits if n else None)
        else:
            dw = d[5 * n + 1:].view(torch.int32)[:n]
            lengths, status = self.encode_vw(d[:n], d[n:2 * n], dw, mask, d[2 * n:3 * n], d[3 * n:4 * n],
                                             stream=stream, mapbits=mapbits)
        return out, d[4 * n:5 * n + 1], lengths, status

    def _encode_tensors_mapped(self, tensors, ptrs, sizes, out, stream, word_sizes, packed, exact):
        """encode_tensors(return_mappings=True): the mappings by mappings_v, then the mapped encode."""
        import torch
        n = len(tensors)
        dev = tensors[0].device if n else torch.device("cuda", self.device)
        dw, mask = None, 0
        parts = [ptrs, sizes]
        if word_sizes is not None and n:
            if isinstance(word_sizes, str):
                if word_sizes != "dtype":
                    raise ValueError('word_sizes is None, "dtype" or one width per tensor')
                widths = np.array([t.element_size() for t in tensors], dtype=np.int32)
            else:
                widths = np.array([int(w) for w in word_sizes], dtype=np.int32)
            if widths.size != n:
                raise ValueError("%d word sizes for %d tensors" % (widths.size, n))
            mask = self.width_mask(widths)
            parts.append(np.concatenate([widths, np.zeros(n % 2, np.int32)]).view(np.int64))
        d = torch.from_numpy(np.concatenate(parts)).to(dev, non_blocking=False)
        if len(parts) == 3:
            dw = d[2 * n:].view(torch.int32)[:n]
        _, bits, _ = self.mappings_v(d[:n], d[n:2 * n], word_sizes=dw, width_mask=mask, stream=stream)
        res = self.encode_tensors(tensors, out=out, stream=stream, word_sizes=word_sizes, packed=packed, exact=exact,
                                  mapbits=bits if n else None)
        return (*res, bits)

    def decode_tensors(self, blobs, offsets, in_lengths, outs, stream=None):
        """Decode blob i = blobs[offsets[i]:offsets[i]+in_lengths[i]] into the preallocated
        contiguous GPU tensor outs[i] (capacity: its byte size).  Returns (lengths, status)."""
        import torch
        optrs, osizes = self._tensor_table(outs)
        n = len(outs)
        d = torch.from_numpy(np.concatenate([optrs, osizes])).to(blobs.device)
        ptrs = offsets[:n].to(torch.int64) + blobs.data_ptr()
        return self.decode_v(ptrs, in_lengths, d[:n], d[n:], stream=stream)

    def analyze_batch(self, data, offsets, stream=None):
        """Full-sample histograms (n, ws, 256), entropies (n, ws), mapping (n, ws), status."""
        import torch
        n = offsets.numel() - 1
        ws = self.config.word_size
        hist = torch.empty((max(n, 1), ws, 256), dtype=torch.int32, device=data.device)
        ent = torch.empty((max(n, 1), ws), dtype=torch.float64, device=data.device)
        mp = torch.empty((max(n, 1), ws), dtype=torch.int32, device=data.device)
        st = torch.empty(max(n, 1), dtype=torch.int32, device=data.device)
        check(self._lib.tdt_analyze_batch(self._h, _ptr(data), _ptr(offsets), n, _ptr(hist), _ptr(ent), _ptr(mp),
                                          _ptr(st), self._stream(stream)))
        return hist[:n], ent[:n], mp[:n], st[:n]

    def error_flags(self, stream=None) -> int:
        """Device invariant flags (tdt_ctx_error_flags; 0 for a correct build).  Synchronises
        the stream the batches were issued on (default: the current torch stream)."""
        fl = C.c_uint32(0)
        check(self._lib.tdt_ctx_error_flags(self._h, self._stream(stream), C.byref(fl)))
        return int(fl.value)

    def set_option(self, option: int, value: int):
        """tdt_ctx_set_option (tuning / diagnostic knobs; results are the same bytes): the TDT_OPT_*
        values of psyne_amd._lib.  TDT_OPT_LARGE_MIN and TDT_OPT_TILE_CAP govern the tiled paths of every
        word size; TDT_OPT_ANY_TILED = 0 keeps every generic-width message on one workgroup, and
        TDT_OPT_ANY_DEC_TILED = 0 every generic-width blob."""
        check(self._lib.tdt_ctx_set_option(self._h, option, int(value)))

    def stat(self, name) -> int:
        """tdt_ctx_get_stat: a name of psyne_amd._lib.STATS ("ANY_DEC_LARGE", "ANY_DEC_BLOCKS",
        "ANY_DEC_TILES": what the generic-width decode's plan claimed in the most recent call whose
        snapshot has landed — synchronise first; "ANY_DEC_BUDGET_LARGE", "ANY_DEC_BUDGET_TILES": the
        current budgets) or a TDT_STAT_* value."""
        from ._lib import STATS
        v = C.c_uint64(0)
        check(self._lib.tdt_ctx_get_stat(self._h, STATS[name] if isinstance(name, str) else int(name), C.byref(v)))
        return int(v.value)

    # ---- host path (socket buffers) -------------------------------------------------------
    def encode_host(self, data: np.ndarray, offsets: np.ndarray):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        # (the host calls ignore TDT_OPT_RAW_FALLBACK: their blobs reach the TDT bound, unless the host
        # option bounds them by n + 4 — tdt_ctx_host_encode_bound)
        sizes = np.diff(offsets.astype(np.int64))
        cap = int((sizes + 4 if self.host_raw_fallback else self._tdt_bounds(sizes, self.config.word_size)).sum()) if n else 0
        out = np.empty(max(cap, 1), np.uint8)
        out_off = np.zeros(n + 1, np.uint64)
        st = np.zeros(max(n, 1), np.int32)
        check(self._lib.tdt_encode_host(self._h, data.ctypes.data, offsets.ctypes.data, n, out.ctypes.data, cap,
                                        out_off.ctypes.data, st.ctypes.data))
        return out[: int(out_off[-1])], out_off, st[:n]

    def decode_host(self, blobs: np.ndarray, offsets: np.ndarray, capacity: int):
        blobs = np.ascontiguousarray(blobs, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        out = np.empty(max(capacity, 1), np.uint8)
        out_off = np.zeros(n + 1, np.uint64)
        st = np.zeros(max(n, 1), np.int32)
        check(self._lib.tdt_decode_host(self._h, blobs.ctypes.data, offsets.ctypes.data, n, out.ctypes.data,
                                        capacity, out_off.ctypes.data, st.ctypes.data))
        return out[: int(out_off[-1])], out_off, st[:n]


class TDTCompressionProtocol:
    """psyne::protocol::TDTCompressionProtocol (tdt_compression.hpp:176-638) on the GPU.

    Same method names, defaults and semantics; encode/decode move one message through the
    C ABI's host path (H2D, kernel, D2H).  Errors raise RuntimeError with the reference's
    messages ("TDT: Invalid encoded data size", "Invalid TDT magic number")."""

    def __init__(self, config: TDTConfig | None = None, device: int = 0, host_raw_fallback: bool = False):
        """host_raw_fallback=True: encode returns "UNCP" + the message where the TDT blob would be longer
        (TDT_OPT_HOST_RAW_FALLBACK); such a message updates the ratio and time metrics no more than one
        the policy routes to UNCP does."""
        self.config_ = config or TDTConfig()
        self.codec = TdtCodec(self.config_, device, host_raw_fallback=host_raw_fallback)
        self._bandwidth = 100.0   # :352
        self._latency = 1.0       # :353
        self._cpu = 0.5           # :354
        self.last_compression_ratio_ = 1.0
        self.last_encode_time_ms_ = 0.0
        self.last_decode_time_ms_ = 0.0
        self.avg_entropy_ = 0.0

    # PROTOCOL CONCEPT ---------------------------------------------------------------------
    def should_transform(self, data, size: int) -> bool:
        return self.codec.should_transform(size)

    def _is_tensor_data(self, size: int) -> bool:  # :409-413
        return size % 4 == 0 and size >= 64

    def analyze_data(self, data, size: int) -> None:
        """analyze_data :206-222, full sample, on the GPU (tdt_analyze_batch)."""
        import torch
        if not self._is_tensor_data(size):
            return
        ws = self.config_.word_size
        words = size // ws
        if words == 0:
            self.avg_entropy_ = 0.0
            return
        buf = np.frombuffer(bytes(memoryview(data)[: words * ws]), dtype=np.uint8)
        d = torch.from_numpy(buf.copy()).cuda(self.codec.device)
        off = torch.tensor([0, words * ws], dtype=torch.int64, device=d.device)
        _, ent, _, st = self.codec.analyze_batch(d, off)
        e = ent[0].cpu().numpy()
        total = 0.0
        for b in range(ws):
            total += float(e[b])
        self.avg_entropy_ = total / ws

    def encode(self, data, size: int | None = None) -> bytes:
        t0 = time.perf_counter()
        buf = bytes(memoryview(data)) if size is None else bytes(memoryview(data)[:size])
        n = len(buf)
        arr = np.frombuffer(buf, dtype=np.uint8) if n else np.zeros(1, np.uint8)
        out, _, st = self.codec.encode_host(arr[:n] if n else arr[:0], np.array([0, n], np.uint64))
        if int(st[0]) != 0:
            raise TdtError(int(st[0]), "encode")
        blob = out.tobytes()
        ratio = transformation_ratio_of(blob, n)
        if ratio is not None:  # compressed: metrics as :243-248
            self.last_compression_ratio_ = ratio
            self.last_encode_time_ms_ = (time.perf_counter() - t0) * 1e3
        return blob

    def decode(self, encoded: bytes) -> bytes:
        t0 = time.perf_counter()
        if len(encoded) < 4:
            raise RuntimeError("TDT: Invalid encoded data size")
        arr = np.frombuffer(bytes(encoded), dtype=np.uint8)
        off = np.array([0, arr.size], np.uint64)
        magic = int.from_bytes(encoded[:4], "little")
        if magic == MAGIC_UNCP:
            cap = arr.size - 4
        elif magic == MAGIC_TDT and arr.size >= 8:
            cap = int.from_bytes(encoded[4:8], "little")
        else:
            cap = 0
        out, _, st = self.codec.decode_host(arr, off, cap)
        s = int(st[0])
        if s != 0:
            msg = _lib.load().tdt_status_string(s).decode()
            raise RuntimeError(msg)
        if magic != MAGIC_UNCP:
            self.last_decode_time_ms_ = (time.perf_counter() - t0) * 1e3
        return out.tobytes()

    def update_network_metrics(self, bandwidth_mbps: float, latency_ms: float) -> None:
        self._bandwidth, self._latency = bandwidth_mbps, latency_ms
        self.codec.set_metrics(self._bandwidth, self._latency, self._cpu)

    def update_system_metrics(self, cpu_usage: float) -> None:
        self._cpu = cpu_usage
        self.codec.set_metrics(self._bandwidth, self._latency, self._cpu)

    # IDENTITY ------------------------------------------------------------------------------
    def protocol_name(self) -> str:
        return "TDT-Compression"

    def is_lossless(self) -> bool:
        return True

    def transformation_ratio(self) -> float:
        return self.last_compression_ratio_

    def processing_overhead_ms(self) -> float:
        return (self.last_encode_time_ms_ + self.last_decode_time_ms_) / 2.0

    def get_average_entropy(self) -> float:
        return self.avg_entropy_

    def get_bandwidth_mbps(self) -> float:
        return self._bandwidth

    def get_cpu_usage(self) -> float:
        return self._cpu
