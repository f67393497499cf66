"""bitar_amd -- MI355X-native segment codec engine (Python host side).

The product is libbitar_hip.so (C ABI in include/bitar_hip.h, HIP kernels in csrc/); the
bitar-shaped C++ front-end lives in cpp/.  This module binds the C ABI with ctypes for the
Python callers (tests, bench.py, __graft_entry__).  torch is used only as plumbing:
device memory and streams.  There is no CPU fallback: if the HIP library is missing or
no gfx950 device is visible, the calls raise.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BITAR_HIP_LIB") or os.path.join(_HERE, "lib", "libbitar_hip.so")

CODEC_LZ4 = 1
CODEC_DEFLATE = 2
CODEC_ZSTD = 3
CODEC_DEFLATE_DYNAMIC = 4  # HuffmanEncoding::DYNAMIC (decoded as CODEC_DEFLATE)
CODEC_LZ4_WIDE = 5  # LZ4 blocks from the wide parse (16 KiB history): the ratio operating point
CODEC_SNAPPY = 6  # one raw Snappy stream per segment (the LZ4 parse; decodes stock raw Snappy)
CODEC_RANS = 72   # order-0 rANS, 64 interleaved states per segment (its own format)
CODEC_SYMTAB = 88  # per-segment symbol table for string data (its own format)
# The column codecs: name -> (base id, high nibble of a stream's byte 0, element widths in bytes).
# The id of a width is base + log2(width): CODEC_<NAME><8 * width>, e.g. CODEC_INTPACK32 = 10,
# and any id of a family decodes all its widths -- except RANSPLANE's, which decode their own
# width alone (the decoder's LDS is sized by the width).
#   INTPACK   frame-of-reference bit packing of integers
#   FLTPACK   decimal-scaled bit packing of floats / doubles
#   DICTPACK  per-segment dictionary + bit-packed indices
#   RUNPACK   per-segment run lengths
#   AUTOPACK  per segment the smallest of the applicable four above (no format of its own: any id
#             decodes all of them)
#   CASCADE   RUNPACK's runs, their values and lengths packed by INTPACK (no candidate of AUTOPACK)
#   RANSPLANE RANS with one table per byte plane of the element (likewise; width 1 is CODEC_RANS)
#   PATCHPACK INTPACK with per-miniblock exceptions for outliers (likewise)
#   DECPACK   INTPACK's packing for 16-byte integers, Arrow decimal128 (likewise; its id is one of
#             the ids from 256 on, include/bitar_hip_codecs.h)
COLUMN_CODECS = {
    "INTPACK": (8, 4, (1, 2, 4, 8)),
    "FLTPACK": (16, 5, (4, 8)),
    "DICTPACK": (24, 6, (4, 8, 16)),
    "RUNPACK": (32, 7, (1, 2, 4, 8, 16)),
    "AUTOPACK": (40, None, (1, 2, 4, 8, 16)),
    "CASCADE": (64, 8, (1, 2, 4, 8)),
    "RANSPLANE": (80, 0xB, (2, 4, 8)),
    "PATCHPACK": (104, 9, (1, 2, 4, 8)),
    "DECPACK": (256, 0xD, (16,)),
}
_COLUMN_IDS = {name: {w: base + w.bit_length() - 1 for w in widths}
               for name, (base, _, widths) in COLUMN_CODECS.items()}
globals().update({f"CODEC_{name}{8 * w}": i for name, ids in _COLUMN_IDS.items()
                  for w, i in ids.items()})
SEGMENT_ERROR = 0xFFFFFFFF
CHECKSUM_CRC32, CHECKSUM_ADLER32, CHECKSUM_CRC32_ADLER32 = 1, 2, 3
MAX_SEG_SIZE = 65536
FILTER_SHUFFLE, FILTER_BITSHUFFLE = 1, 2  # bitar_hip_filter (element widths 2, 4, 8, 16)
# whole-buffer raw Snappy streams (include/bitar_hip_snappy.h): the fragment size,
# bitar_hip_snappy_split_status, and the bit of max_rounds that forbids the serial finish
SNAPPY_BLOCK = 65536
SNAPPY_SPLIT_OK, SNAPPY_SPLIT_UNSUPPORTED, SNAPPY_SPLIT_INVALID, SNAPPY_SPLIT_INCOMPLETE = range(4)
SNAPPY_NO_SERIAL_FINISH = 0x80000000
# bitar_hip_config.flags (initial decoder options of a context)
FLAG_INFLATE_WAVE_ONLY, FLAG_ZSTD_WAVE_ONLY, FLAG_ZSTD_LANE_EXEC, FLAG_COUNT_PATHS = 1, 2, 4, 8
FLAG_PLAIN_ORDER = 0x10  # segment i is workgroup i (no cost-ordered dispatch; same output)
FLAG_ZSTD_SERIAL = 0x20  # Zstd literals and phase A in series (default: side by side)
# bitar_hip_debug_order: the modes, the slot count "what an LZ4 compress call would get", the tag
# of a fast lane's entry, and the status of a call that runs in plain order
ORDER_COMPRESS_KEY, ORDER_DECOMPRESS_KEY, ORDER_CALLER_KEYS = 0, 1, 2
ORDER_SLOTS_CALL = 0xFFFFFFFF
ORDER_LANE_TAG = 0x80000000
NO_ORDER = 1
# bitar_hip_path_counter indices
PATHS = ("inflate_wave", "inflate_wave_reject", "inflate_batch_segs", "inflate_batches",
         "zstd_wave", "zstd_handed", "zstd_seqdec", "zstd_seqdec_reject", "zstd_exec",
         "zstd_exec_reject", "lz4_far",
         # LZ4 batch diagnostics (a -DBITAR_LZ4D_PROFILE=1 build only)
         "lz4_batches", "lz4_batch_bytes", "lz4_general_seqs", "lz4_stop_parse",
         "lz4_stop_ineligible")
PATH_COUNT = 16


class DecoderOptions(ctypes.Structure):
    """bitar_hip_decoder_options (include/bitar_hip.h)"""
    _fields_ = [("inflate_lanes", ctypes.c_uint32), ("zstd_lanes", ctypes.c_uint32),
                ("zstd_seq", ctypes.c_uint32), ("count_paths", ctypes.c_uint32)]

# negated arrow::StatusCode (reference src/include/util.h:157-205)
STATUS_NAMES = {0: "OK", -1: "OutOfMemory", -4: "Invalid", -5: "IOError", -6: "CapacityError",
                -8: "Cancelled", -9: "UnknownError", -10: "NotImplemented"}


class BitarError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code


_lib = None


def build(verbose=False):
    """Compile libbitar_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    import subprocess
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-s", "-j8", "-C", _HERE], stdout=out)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BitarError(-10, f"{LIB_PATH} is not built (run bitar_amd.build())")
    L = ctypes.CDLL(LIB_PATH)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    sig = {
        "bitar_hip_abi_version": (i32, []),
        "bitar_hip_last_error": (ctypes.c_char_p, []),
        "bitar_hip_device_count": (i32, [ctypes.POINTER(i32)]),
        "bitar_hip_open": (i32, [i32, vp, ctypes.POINTER(vp)]),
        "bitar_hip_close": (i32, [vp]),
        "bitar_hip_stream": (i32, [vp, u32, ctypes.POINTER(vp)]),
        "bitar_hip_device": (i32, [vp, ctypes.POINTER(i32)]),
        "bitar_hip_slot_size": (u64, [u32, u32]),
        "bitar_hip_max_distance": (u32, [u32]),
        "bitar_hip_alloc": (i32, [vp, u64, ctypes.POINTER(vp)]),
        "bitar_hip_free": (i32, [vp, vp]),
        "bitar_hip_host_alloc": (i32, [vp, u64, ctypes.POINTER(vp)]),
        "bitar_hip_host_free": (i32, [vp, vp]),
        "bitar_hip_memcpy": (i32, [vp, vp, vp, u64, vp]),
        "bitar_hip_compress": (i32, [vp, vp, u32, vp, u64, u32, vp, u64, vp]),
        "bitar_hip_compress_scattered": (i32, [vp, vp, u32, vp, u64, u32, vp, u64, vp]),
        "bitar_hip_pointer_info": (i32, [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        "bitar_hip_decompress": (i32, [vp, vp, u32, vp, vp, u32, u32, vp, u64, vp]),
        "bitar_hip_decompress_slab": (i32, [vp, vp, u32, vp, u64, vp, u32, u32, vp, u64, vp]),
        "bitar_hip_sync": (i32, [vp, vp]),
        "bitar_hip_pack": (i32, [vp, vp, vp, u64, vp, u32, vp, vp]),
        "bitar_hip_pack_lz4f": (i32, [vp, vp, vp, u64, u32, vp, u64, vp, vp, vp, vp]),
        "bitar_hip_fill": (i32, [vp, vp, i32, u64, vp, u64]),
        "bitar_hip_fill_at": (i32, [vp, vp, i32, u64, u64, vp, u64]),
        "bitar_hip_checksum": (i32, [vp, vp, u32, vp, u64, u32, vp, u32, vp]),
        "bitar_hip_copy_batch": (i32, [vp, vp, vp, vp, vp, u32]),
        "bitar_hip_lz4_chain": (i32, [vp, vp, vp, u32, vp, u32, vp, u64, vp]),
        "bitar_hip_get_decoder_options": (i32, [vp, ctypes.POINTER(DecoderOptions)]),
        "bitar_hip_set_decoder_options": (i32, [vp, ctypes.POINTER(DecoderOptions)]),
        "bitar_hip_path_counters": (i32, [vp, ctypes.POINTER(ctypes.c_uint64), u32]),
        "bitar_hip_compress_host": (i32, [vp, vp, u32, vp, u64, u32, vp, vp, vp, u64, vp]),
        "bitar_hip_decompress_host": (i32, [vp, vp, u32, vp, vp, u32, u32, vp, vp, u64, vp]),
        "bitar_hip_compress_bits": (i32, [vp, vp, u32, vp, u64, u32, vp, u64, vp, vp]),
        "bitar_hip_deflate_join": (i32, [vp, vp, vp, u64, vp, vp, u32, vp, vp, u64]),
        "bitar_hip_deflate_split": (i32, [vp, vp, vp, u64, vp, vp, u32, vp, u64, vp]),
        "bitar_hip_crc32_combine": (i32, [vp, vp, vp, u64, u32, u32, vp]),
        "bitar_hip_filter_apply": (i32, [vp, vp, u32, u32, vp, u64, u32, vp, u32, vp]),
        "bitar_hip_filter_invert": (i32, [vp, vp, u32, u32, vp, u64, u32, vp, u32, vp]),
        "bitar_hip_debug_order": (i32, [vp, vp, u32, vp, u64, u32, vp, u32, u32, u32, vp, vp,
                                        ctypes.POINTER(u32)]),
        "bitar_hip_snappy_join": (i32, [vp, vp, vp, u64, vp, u64, u32, vp, vp, u64, vp]),
        "bitar_hip_snappy_split": (i32, [vp, vp, vp, u64, u64, u32, vp, vp, vp]),
        "bitar_hip_snappy_decompress_joined": (i32, [vp, vp, vp, u64, u64, vp, vp, u64, vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


# every symbol include/bitar_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = ("bitar_hip_abi_version", "bitar_hip_last_error", "bitar_hip_device_count",
               "bitar_hip_open", "bitar_hip_close", "bitar_hip_stream", "bitar_hip_device",
               "bitar_hip_slot_size", "bitar_hip_max_distance", "bitar_hip_alloc", "bitar_hip_free",
               "bitar_hip_host_alloc", "bitar_hip_host_free", "bitar_hip_memcpy",
               "bitar_hip_compress", "bitar_hip_compress_scattered", "bitar_hip_pointer_info",
               "bitar_hip_decompress", "bitar_hip_decompress_slab",
               "bitar_hip_sync", "bitar_hip_pack", "bitar_hip_pack_lz4f", "bitar_hip_fill",
               "bitar_hip_fill_at", "bitar_hip_checksum", "bitar_hip_copy_batch",
               "bitar_hip_lz4_chain", "bitar_hip_get_decoder_options",
               "bitar_hip_set_decoder_options", "bitar_hip_path_counters",
               "bitar_hip_compress_host", "bitar_hip_decompress_host",
               "bitar_hip_compress_bits", "bitar_hip_deflate_join", "bitar_hip_deflate_split",
               "bitar_hip_crc32_combine", "bitar_hip_filter_apply", "bitar_hip_filter_invert",
               "bitar_hip_debug_order")
# every symbol include/bitar_hip_snappy.h declares (whole-buffer raw Snappy streams: additive, a
# header of their own; checked by tests/test_gpu_snappy_codec.py)
SNAPPY_STREAM_SYMBOLS = ("bitar_hip_snappy_join", "bitar_hip_snappy_split",
                         "bitar_hip_snappy_decompress_joined")


def check(rc):
    if rc != 0:
        raise BitarError(rc, lib().bitar_hip_last_error().decode())
    return rc


def slot_size(codec, seg):
    return int(lib().bitar_hip_slot_size(codec, seg))


def _column_codec(name, width):
    try:
        return _COLUMN_IDS[name][width]
    except (KeyError, TypeError):
        *most, last = map(str, COLUMN_CODECS[name][2])
        widths = f"{', '.join(most)} or {last}" if most else last
        raise ValueError(f"{name} element width must be {widths}, not {width!r}") from None


def codec_intpack(width):
    """the INTPACK codec id of an element width of 1, 2, 4 or 8 bytes"""
    return _column_codec("INTPACK", width)


def codec_fltpack(width):
    """the FLTPACK codec id of an element width of 4 (float32) or 8 (float64) bytes"""
    return _column_codec("FLTPACK", width)


def codec_dictpack(width):
    """the DICTPACK codec id of an element width of 4, 8 or 16 bytes"""
    return _column_codec("DICTPACK", width)


def codec_runpack(width):
    """the RUNPACK codec id of an element width of 1, 2, 4, 8 or 16 bytes"""
    return _column_codec("RUNPACK", width)


def codec_autopack(width):
    """the AUTOPACK codec id of an element width of 1, 2, 4, 8 or 16 bytes"""
    return _column_codec("AUTOPACK", width)


def codec_cascade(width):
    """the CASCADE codec id of an element width of 1, 2, 4 or 8 bytes"""
    return _column_codec("CASCADE", width)


def codec_patchpack(width):
    """the PATCHPACK codec id of an element width of 1, 2, 4 or 8 bytes"""
    return _column_codec("PATCHPACK", width)


def codec_decpack(width):
    """the DECPACK codec id of an element width of 16 bytes (Arrow decimal128)"""
    return _column_codec("DECPACK", width)


def codec_ransplane(width):
    """the RANSPLANE codec id of an element width of 2, 4 or 8 bytes"""
    return _column_codec("RANSPLANE", width)


def max_distance(codec):
    """largest match distance the encoder of `codec` emits (its window's reach)"""
    return int(lib().bitar_hip_max_distance(codec))


def device_count():
    n = ctypes.c_int(0)
    check(lib().bitar_hip_device_count(ctypes.byref(n)))
    return n.value


def _ptr(t):
    """device pointer of a torch tensor (or an int address, or None)."""
    if t is None:
        return None
    if isinstance(t, int):
        return ctypes.c_void_p(t)
    return ctypes.c_void_p(t.data_ptr())


class Engine:
    """One context on one gfx950 device: the CompressDevice analogue.

    Calls are asynchronous on `stream` (default: torch's current stream on that device, so
    torch copies and our kernels stay ordered).  Buffers are torch uint8 tensors in HBM.
    """

    def __init__(self, device=0, num_streams=1, flags=0):
        import torch  # plumbing only
        self.torch = torch
        self.device = device

        class Cfg(ctypes.Structure):
            _fields_ = [("num_streams", ctypes.c_uint32), ("flags", ctypes.c_uint32)]

        cfg = Cfg(num_streams, flags)
        ctx = ctypes.c_void_p()
        check(lib().bitar_hip_open(device, ctypes.byref(cfg), ctypes.byref(ctx)))
        self.ctx = ctx

    def close(self):
        if self.ctx:
            lib().bitar_hip_close(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self, stream):
        if stream is None:
            return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)
        if isinstance(stream, int):
            return ctypes.c_void_p(stream)
        return ctypes.c_void_p(stream.cuda_stream)

    def decoder_options(self):
        o = DecoderOptions()
        check(lib().bitar_hip_get_decoder_options(self.ctx, ctypes.byref(o)))
        return {f: getattr(o, f) for f, _ in DecoderOptions._fields_}

    def set_decoder_options(self, **kw):
        """change this context's decoders (inflate_lanes / zstd_lanes / zstd_seq /
        count_paths); returns the previous options"""
        old = self.decoder_options()
        new = dict(old, **kw)
        check(lib().bitar_hip_set_decoder_options(
            self.ctx, ctypes.byref(DecoderOptions(*(new[f] for f, _ in DecoderOptions._fields_)))))
        return old

    def path_counters(self):
        """{path: segments} since the last call (waits for the device, then resets)"""
        v = (ctypes.c_uint64 * PATH_COUNT)()
        check(lib().bitar_hip_path_counters(self.ctx, v, PATH_COUNT))
        return {name: int(v[k]) for k, name in enumerate(PATHS)}

    def queue_pair_stream(self, qp):
        s = ctypes.c_void_p()
        check(lib().bitar_hip_stream(self.ctx, qp, ctypes.byref(s)))
        return s.value

    def empty(self, nbytes, dtype=None):
        t = self.torch
        return t.empty(nbytes, dtype=dtype or t.uint8, device=f"cuda:{self.device}")

    # --- hot path ------------------------------------------------------------------
    def compress_into(self, codec, data, seg, slab, stride, sizes, n=None, stream=None):
        n = data.numel() * data.element_size() if n is None else n
        check(lib().bitar_hip_compress(self.ctx, self._stream(stream), codec, _ptr(data), n, seg,
                                       _ptr(slab), stride, _ptr(sizes)))

    def compress_host_into(self, codec, host, n, seg, stage, slab, stride, sizes, stream=None):
        """compress n bytes of host memory (a pinned torch CPU tensor, or an address) through
        the HBM staging tensor `stage`, link and kernels overlapped"""
        check(lib().bitar_hip_compress_host(self.ctx, self._stream(stream), codec, _ptr(host),
                                            n, seg, _ptr(stage), _ptr(slab), None, stride,
                                            _ptr(sizes)))

    def decompress_host_into(self, codec, srcs, sizes, nseg, seg, stage, host, produced,
                             capacity=None, stream=None):
        """decompress into host memory (nseg*seg bytes at `host`) through `stage`"""
        cap = nseg * seg if capacity is None else capacity
        check(lib().bitar_hip_decompress_host(self.ctx, self._stream(stream), codec, _ptr(srcs),
                                              _ptr(sizes), nseg, seg, _ptr(stage), _ptr(host),
                                              cap, _ptr(produced)))

    def decompress_slab_into(self, codec, slab, stride, sizes, nseg, seg, out, produced,
                             capacity=None, stream=None):
        cap = out.numel() if capacity is None else capacity
        check(lib().bitar_hip_decompress_slab(self.ctx, self._stream(stream), codec, _ptr(slab),
                                              stride, _ptr(sizes), nseg, seg, _ptr(out), cap,
                                              _ptr(produced)))

    def decompress_into(self, codec, srcs, sizes, nseg, seg, out, produced, capacity=None,
                        stream=None):
        """srcs: device int64 tensor of segment addresses."""
        cap = out.numel() if capacity is None else capacity
        check(lib().bitar_hip_decompress(self.ctx, self._stream(stream), codec, _ptr(srcs),
                                         _ptr(sizes), nseg, seg, _ptr(out), cap, _ptr(produced)))

    def pack(self, slab, stride, sizes, nseg, offsets, frame=None, stream=None):
        check(lib().bitar_hip_pack(self.ctx, self._stream(stream), _ptr(slab), stride,
                                   _ptr(sizes), nseg, _ptr(offsets), _ptr(frame)))

    def pack_lz4f(self, data, n, seg, slab, stride, sizes, framed, offsets, frame=None,
                  stream=None):
        """the data blocks of an LZ4 frame from the slots of a CODEC_LZ4 compress of n bytes at
        segment size seg: framed (int32 tensor, nseg) the blocks' sizes with their size fields,
        offsets (int64 tensor, nseg + 1) their exclusive prefix sum, frame (uint8 tensor, or
        None: sizes only, data and slab are not read)"""
        check(lib().bitar_hip_pack_lz4f(self.ctx, self._stream(stream), _ptr(data), n, seg,
                                        _ptr(slab), stride, _ptr(sizes), _ptr(framed),
                                        _ptr(offsets), _ptr(frame)))

    def fill(self, kind, seed, out, n=None, stream=None, offset=0):
        """bytes [offset, offset + n) of the synthetic stream `kind` into `out`."""
        n = out.numel() if n is None else n
        check(lib().bitar_hip_fill_at(self.ctx, self._stream(stream), kind, seed, offset,
                                      _ptr(out), n))

    def checksum(self, kind, data, seg, sums, n=None, lens=None, nseg=None, stream=None):
        """per-segment CRC32 / Adler32 (uint64 tensor `sums`) of uncompressed data"""
        n = data.numel() if n is None else n
        nseg = (n + seg - 1) // seg if nseg is None else nseg
        check(lib().bitar_hip_checksum(self.ctx, self._stream(stream), kind, _ptr(data), n, seg,
                                       _ptr(lens), nseg, _ptr(sums)))

    # --- shuffle / bitshuffle of fixed-width column buffers, per segment ------------------
    def _filter(self, fn, filter, width, data, seg, out, n, lens, nseg, stream):
        n = data.numel() * data.element_size() if n is None else n
        nseg = (n + seg - 1) // seg if nseg is None and seg > 0 else nseg or 0
        check(fn(self.ctx, self._stream(stream), filter, width, _ptr(data), n, seg, _ptr(lens),
                 nseg, _ptr(out)))

    def filter_into(self, filter, width, data, seg, out, n=None, lens=None, nseg=None,
                    stream=None):
        """segment i of `data` (lens[i] bytes, or min(seg, n - i*seg)) filtered into `out` at
        the same offset: FILTER_SHUFFLE or FILTER_BITSHUFFLE of `width`-byte elements"""
        self._filter(lib().bitar_hip_filter_apply, filter, width, data, seg, out, n, lens, nseg,
                     stream)

    def unfilter_into(self, filter, width, data, seg, out, n=None, lens=None, nseg=None,
                      stream=None):
        """the inverse of filter_into (lens: e.g. the produced sizes of a decompress)"""
        self._filter(lib().bitar_hip_filter_invert, filter, width, data, seg, out, n, lens, nseg,
                     stream)

    # --- one DEFLATE stream from the segments' streams (gzip members) -------------------
    def compress_bits_into(self, codec, data, seg, slab, stride, sizes, bits, n=None,
                           stream=None):
        """compress_into for the two DEFLATE codecs, + each segment's exact bit length in the
        int32 tensor `bits` (None: exactly compress_into)"""
        n = data.numel() * data.element_size() if n is None else n
        check(lib().bitar_hip_compress_bits(self.ctx, self._stream(stream), codec, _ptr(data), n,
                                            seg, _ptr(slab), stride, _ptr(sizes), _ptr(bits)))

    def deflate_join(self, slab, stride, sizes, bits, nseg, starts, joined=None, capacity=None,
                     stream=None):
        """starts (int64 tensor, nseg + 1): each segment's bit position in the one raw DEFLATE
        stream joined from the slots; joined (uint8 tensor or None: positions only)"""
        # (capacity: a multiple of 4, the stream is written in whole dwords)
        cap = (joined.numel() & ~3 if joined is not None else 0) if capacity is None else capacity
        check(lib().bitar_hip_deflate_join(self.ctx, self._stream(stream), _ptr(slab), stride,
                                           _ptr(sizes), _ptr(bits), nseg, _ptr(starts),
                                           _ptr(joined), cap))

    def deflate_split(self, joined, joined_len, starts, entries, nseg, slab, stride, sizes,
                      stream=None):
        """the inverse of deflate_join: entries (int32 tensor) = bits | stored << 23"""
        check(lib().bitar_hip_deflate_split(self.ctx, self._stream(stream), _ptr(joined),
                                            joined_len, _ptr(starts), _ptr(entries), nseg,
                                            _ptr(slab), stride, _ptr(sizes)))

    def crc32_combine(self, sums, n, seg, crc, stream=None):
        """crc (int32 tensor, 1 entry) = CRC-32 of n bytes from their segments' CRC-32s"""
        check(lib().bitar_hip_crc32_combine(self.ctx, self._stream(stream), _ptr(sums), n, seg,
                                            (n + seg - 1) // seg, _ptr(crc)))

    # --- one raw Snappy stream from the segments' streams, and back -------
    def snappy_join(self, slab, stride, sizes, n, offsets, joined=None, capacity=None,
                    joined_len=None, seg=SNAPPY_BLOCK, stream=None):
        """the slots of a CODEC_SNAPPY compress of n bytes at 64 KiB segments as ONE raw Snappy
        stream in `joined` (uint8 tensor, or None: sizes only); offsets (int64 tensor, nseg + 1):
        the exclusive prefix sum of the segments' body sizes; joined_len (int64 tensor, 1
        entry, or None): the stream's length"""
        cap = (joined.numel() if joined is not None else 0) if capacity is None else capacity
        check(lib().bitar_hip_snappy_join(self.ctx, self._stream(stream), _ptr(slab), stride,
                                          _ptr(sizes), n, seg, _ptr(offsets), _ptr(joined), cap,
                                          _ptr(joined_len)))

    def snappy_split(self, joined, length, n, starts, status, max_rounds=0, stats=None,
                     stream=None):
        """starts (int64 tensor, ceil(n / 65536) + 1): where each 64 KiB block of output begins
        in the raw Snappy stream joined[:length] that declares n bytes, and `length` last;
        status (int32 tensor, 1 entry): SNAPPY_SPLIT_*; stats (int32 tensor, 4 entries, or
        None): rounds, tile walks, tiles, serial finish"""
        check(lib().bitar_hip_snappy_split(self.ctx, self._stream(stream), _ptr(joined), length, n,
                                           max_rounds, _ptr(starts), _ptr(status), _ptr(stats)))

    def decompress_joined_into(self, joined, length, n, starts, out, produced, capacity=None,
                               stream=None):
        """every fragment of the stream between the starts of snappy_split, in one launch:
        fragment k to out[k * 65536:], produced[k] its size or SEGMENT_ERROR"""
        cap = out.numel() if capacity is None else capacity
        check(lib().bitar_hip_snappy_decompress_joined(self.ctx, self._stream(stream),
                                                       _ptr(joined), length, n, _ptr(starts),
                                                       _ptr(out), cap, _ptr(produced)))

    def copy_batch(self, srcs, dsts, sizes, n, stream=None):
        """entry i: sizes[i] bytes from srcs[i] to dsts[i] (int64 / int32 device tensors)"""
        check(lib().bitar_hip_copy_batch(self.ctx, self._stream(stream), _ptr(srcs), _ptr(dsts),
                                         _ptr(sizes), n))

    def autopack_census(self, slab, stride, sizes, nseg):
        """what an AUTOPACK slab is made of: {"INTPACK", "FLTPACK", "DICTPACK", "RUNPACK": the
        segments packed in that format, "stored": those in any format's stored form, "other":
        empty streams and tags of no format}.  Reads the tag bytes only (a strided view of the
        slab on torch's current stream); waits for them."""
        t = self.torch
        formats = {nibble: name for name, (_, nibble, _) in COLUMN_CODECS.items()
                   if nibble and nibble <= 7}  # (AUTOPACK's four)
        if nseg == 0:
            return {k: 0 for k in (*formats.values(), "stored", "other")}
        tags = t.as_strided(slab, (nseg,), (stride,)).to(t.int64)
        nib = tags >> 4
        live = sizes[:nseg] != 0
        # INTPACK and FLTPACK store with mode 2 in bits 2..3, DICTPACK and RUNPACK with bit 3
        stored = t.where(nib <= 5, (tags >> 2 & 3) == 2, (tags >> 3 & 1) == 1)
        known = live & (nib >= 4) & (nib <= 7)
        out = {name: int((known & ~stored & (nib == k)).sum()) for k, name in formats.items()}
        out["stored"] = int((known & stored).sum())
        out["other"] = nseg - int(known.sum())
        return out

    def lz4_chain(self, src, src_len, blocks, nblocks, out, capacity, produced, stream=None):
        """the linked blocks of one LZ4 frame, in order on one wavefront (bitar_hip_lz4_chain):
        blocks = nblocks pairs {offset in src, size | 1 << 31 when stored} of uint32 in HBM;
        produced[0] receives the size or SEGMENT_ERROR (then the next sync raises IOError)"""
        check(lib().bitar_hip_lz4_chain(self.ctx, self._stream(stream), _ptr(src), src_len,
                                        _ptr(blocks), nblocks, _ptr(out), capacity,
                                        _ptr(produced)))

    def debug_order(self, mode, nseg, data=None, n=0, seg=0, values=None, cut=0, slots=0,
                    keys=False, stream=None):
        """the dispatch order a call of nseg segments builds (bitar_hip_debug_order), for tests:
        -> (order, keys, slots_used).  order: int32 HBM tensor of nseg entries, the fast lanes'
        tagged with ORDER_LANE_TAG (the sign bit), or None where the call runs in plain order;
        keys (keys=True, not for ORDER_DECOMPRESS_KEY): int32 HBM tensor, else None.
        ORDER_COMPRESS_KEY reads n bytes of `data` (a uint8 tensor or an address) in segments of
        seg; the other modes read `values` (int32 tensor: compressed sizes, or keys)."""
        t = self.torch
        order = self.empty(max(nseg, 1), dtype=t.int32)
        kout = self.empty(max(nseg, 1), dtype=t.int32) if keys else None
        used = ctypes.c_uint32(0)
        rc = lib().bitar_hip_debug_order(self.ctx, self._stream(stream), mode, _ptr(data), n, seg,
                                         _ptr(values), nseg, cut, slots, _ptr(order), _ptr(kout),
                                         ctypes.byref(used))
        if rc == NO_ORDER:
            return None, None, used.value
        check(rc)
        return order[:nseg], kout[:nseg] if keys else None, used.value

    def sync(self, stream=None):
        s = self._stream(stream) if stream is not False else None
        check(lib().bitar_hip_sync(self.ctx, s))

    # --- convenience: whole-buffer round trip (the CompressDevice call pair) -----------
    def compress(self, codec, data, seg, stream=None):
        """-> (slab, stride, sizes) ; data: uint8 HBM tensor.  sizes stays on device."""
        n = data.numel()
        nseg = (n + seg - 1) // seg
        stride = slot_size(codec, seg)
        slab = self.empty(max(nseg * stride, 1))
        sizes = self.empty(max(nseg, 1), dtype=self.torch.int32)
        self.compress_into(codec, data, seg, slab, stride, sizes, n=n, stream=stream)
        return slab, stride, sizes[:nseg]

    def decompress(self, codec, slab, stride, sizes, seg, stream=None):
        nseg = sizes.numel()
        out = self.empty(max(nseg * seg, 1))
        produced = self.empty(max(nseg, 1), dtype=self.torch.int32)
        self.decompress_slab_into(codec, slab, stride, sizes, nseg, seg, out, produced,
                                  capacity=nseg * seg, stream=stream)
        return out, produced[:nseg]
