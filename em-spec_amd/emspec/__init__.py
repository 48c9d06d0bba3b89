"""Python binding of libemspec's C ABI (include/emspec.h) via ctypes.

Used by tests/, bench.py and __graft_entry__.py.  The production host side is
the Node addon in em-spec_amd/js/; this module exposes the same calls for the
Python tooling.  There is NO fallback: if libemspec.so is missing or no gfx950
device is present, loading / Engine() raises.
"""
import ctypes as C
import os
import sys

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_PKG)                 # em-spec_amd/
LIB_PATH = os.path.join(ROOT, "libemspec.so")
# the same sources built with -DEMSPEC_DIAG: adds include/emspec_debug.h, the stamped / A-B kernel builds and the
# EMSPEC_* environment switches.  Tools and the tests that probe internals load this one; the product never does.
DIAG_LIB_PATH = os.path.join(ROOT, "libemspec_diag.so")

ABI_VERSION = 2
OK = 0
ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_OOM, ERR_STATE, ERR_COMM = -1, -2, -3, -4, -5, -6
MODE_FAST, MODE_EXACT = 0, 1
COMM_ID_BYTES = 128
GATHER_LOOPBACK = 1
GATHER_PACKED = 2
PCM_S16, PCM_S24, PCM_S32, PCM_F32 = 1, 2, 3, 4
PCM_MAX_CHANNELS = PCM_MAX_VIEWS = 8

SYMBOLS = [
    "emspec_default_config", "emspec_create", "emspec_destroy", "emspec_last_error", "emspec_set_colormap",
    "emspec_num_columns", "emspec_latency_columns", "emspec_column", "emspec_column_flush", "emspec_reset",
    "emspec_batch", "emspec_batch_device", "emspec_parity_dump", "emspec_parity_dump_device",
    "emspec_get_tables", "emspec_device_arch", "emspec_uses_fused", "emspec_set_row_edges_hz",
    "emspec_get_row_edges_hz", "emspec_host_alloc", "emspec_host_free", "emspec_set_display",
    "emspec_push_samples", "emspec_push_columns", "emspec_warped_edges_hz", "emspec_make_colormap",
    "emspec_comm_unique_id", "emspec_comm_init", "emspec_comm_destroy", "emspec_comm_rank", "emspec_comm_world",
    "emspec_gather_columns", "emspec_wire_bound", "emspec_wire_pack", "emspec_wire_unpack", "emspec_batch_gather",
    "emspec_parity_dump_exact", "emspec_gather_packed_layout", "emspec_mode", "emspec_build_info", "emspec_device_status",
    "emspec_comm_set_timeout", "emspec_batch_packed", "emspec_wire_unpack_host",
    "emspec_columns", "emspec_columns_flush", "emspec_push_columns_multi", "emspec_push_samples_multi",
    "emspec_reset_stream", "emspec_live_streams",
    "emspec_multires_columns", "emspec_multires_shift", "emspec_batch_multires", "emspec_batch_multires_device",
    "emspec_pcm_frame_bytes", "emspec_pcm_decode_device", "emspec_batch_pcm", "emspec_batch_pcm_packed",
    "emspec_push_samples_pcm", "emspec_push_samples_pcm_multires",
    "emspec_wave_device", "emspec_wave_host", "emspec_set_wave_out",
    "emspec_peaks_device", "emspec_peaks_host", "emspec_batch_peaks", "emspec_batch_peaks_device", "emspec_position_hz",
    "emspec_set_time_reduce", "emspec_time_reduce", "emspec_reduced_columns",
    "emspec_columns_multires", "emspec_push_columns_multires", "emspec_push_samples_multires",
]
# the multi-resolution live session's entry points: a library built before they existed (tools/live_multires_rate.py times one
# next to this build) loads without them
OPTIONAL_SYMBOLS = SYMBOLS[-3:]
# the time reduction's: likewise (tools/overview_rate.py times the parent commit's library at factor 1)
REDUCE_SYMBOLS = SYMBOLS[-6:-3]
# the spectral peaks': likewise (tools/peaks_rate.py may time a library built before them next to this build)
PEAKS_SYMBOLS = SYMBOLS[-11:-6]
# the waveform envelope's: likewise (tools/wave_rate.py times the parent commit's library next to this build)
WAVE_SYMBOLS = SYMBOLS[-14:-11]
# the multi-band batch's: likewise (tools/multiband_rate.py may load a library built before them); appended behind the slices above
MULTIBAND_SYMBOLS = ["emspec_multiband_shifts", "emspec_multiband_columns", "emspec_batch_multiband", "emspec_batch_multiband_device"]
# the live calls' overlays: likewise (tools/live_rate.py times the parent commit's library next to this build)
LIVE_OVERLAY_SYMBOLS = ["emspec_set_live_peaks", "emspec_set_live_wave"]
# the multi-band live session's: likewise (tools/live_multiband_rate.py times the parent commit's library next to this build)
LIVE_MULTIBAND_SYMBOLS = ["emspec_columns_multiband", "emspec_push_columns_multiband", "emspec_push_samples_multiband",
                          "emspec_push_samples_pcm_multiband"]
# the live history's: likewise (tools/history_rate.py times the parent commit's library next to this build)
HISTORY_SYMBOLS = ["emspec_set_live_history", "emspec_live_history", "emspec_history_view_device", "emspec_history_view"]
# the live audio history's: likewise (tools/live_audio_rate.py times the parent commit's library next to this build)
AUDIO_SYMBOLS = ["emspec_set_live_audio", "emspec_live_audio", "emspec_audio_view_device", "emspec_audio_view",
                 "emspec_audio_batch_device", "emspec_audio_batch"]
# the stereo image's: likewise (tools/stereo_rate.py times the parent commit's library next to this build)
STEREO_SYMBOLS = ["emspec_stereo_default_map", "emspec_make_stereo_colormap", "emspec_set_stereo_colormap", "emspec_stereo_device",
                  "emspec_stereo_host", "emspec_batch_stereo_device", "emspec_batch_pcm_stereo", "emspec_history_view_stereo_device",
                  "emspec_history_view_stereo"]
# the level meters': likewise (tools/level_rate.py times the parent commit's library next to this build)
LEVEL_SYMBOLS = ["emspec_level_device", "emspec_level_host", "emspec_cross_device", "emspec_cross_host", "emspec_set_level_out",
                 "emspec_set_cross_out", "emspec_level_window", "emspec_level_values", "emspec_cross_correlation"]
# the live level meters': likewise (tools/live_rate.py times the parent commit's library next to this build)
LIVE_LEVEL_SYMBOLS = ["emspec_set_live_level", "emspec_set_live_cross", "emspec_level_sum", "emspec_cross_sum"]
SYMBOLS = (SYMBOLS + MULTIBAND_SYMBOLS + LIVE_OVERLAY_SYMBOLS + LIVE_MULTIBAND_SYMBOLS + HISTORY_SYMBOLS + AUDIO_SYMBOLS + STEREO_SYMBOLS
           + LEVEL_SYMBOLS + LIVE_LEVEL_SYMBOLS)
STEREO_PAN_CENTRE, STEREO_PAN_LEVELS = 16, 33
SESSION_MULTI, SESSION_ONE = 0, 1
_SESSIONS = {"multi": SESSION_MULTI, "one": SESSION_ONE, SESSION_MULTI: SESSION_MULTI, SESSION_ONE: SESSION_ONE}


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("rows", C.c_int32), ("mode", C.c_int32),
                ("sample_rate", C.c_float), ("fmin_hz", C.c_float), ("fmax_hz", C.c_float), ("gain", C.c_float),
                ("db_top", C.c_float), ("db_range", C.c_float), ("gate_db", C.c_float), ("power_floor", C.c_float)]


class Out(C.Structure):
    _fields_ = [("db", C.c_void_p), ("rgba", C.c_void_p), ("index", C.c_void_p)]


class ViewMap(C.Structure):
    """emspec_view_map: the colour law of a history view (db_top, db_range, gate_db as in the configuration) and the dB shift
    applied in front of it."""
    _fields_ = [("db_top", C.c_float), ("db_range", C.c_float), ("gate_db", C.c_float), ("shift_db", C.c_float)]


class Level(C.Structure):
    """emspec_level: the sum of k^2 of a window's samples in two limbs (sq_hi 2^32 + sq_lo), the peak |k| and the count of NaN and
    saturated samples; k = the sample in units of 2^-24."""
    _fields_ = [("sq_lo", C.c_uint64), ("sq_hi", C.c_uint64), ("peak", C.c_uint32), ("odd", C.c_uint32)]


class Cross(C.Structure):
    """emspec_cross: the sum of k_A k_B of a pair of streams over a window in two limbs (hi 2^32 + lo)."""
    _fields_ = [("lo", C.c_uint64), ("hi", C.c_int64)]


class StereoMap(C.Structure):
    """emspec_stereo_map: the colour law of a stereo image - db_top, db_range, gate_db and shift_db as in ViewMap, applied to the
    level (the louder channel's dB), and pan_range_db, the dB difference that reads as fully to one side."""
    _fields_ = [("db_top", C.c_float), ("db_range", C.c_float), ("gate_db", C.c_float), ("shift_db", C.c_float),
                ("pan_range_db", C.c_float)]


def _stereo_map(map):
    """None, a StereoMap, a (db_top, db_range, gate_db, shift_db, pan_range_db) tuple or a dict of those names -> StereoMap or
    None."""
    if map is None or isinstance(map, StereoMap):
        return map
    if isinstance(map, dict):
        return StereoMap(float(map["db_top"]), float(map["db_range"]), float(map["gate_db"]), float(map.get("shift_db", 0.0)),
                         float(map.get("pan_range_db", 12.0)))
    return StereoMap(*(float(x) for x in map))


class PcmFormat(C.Structure):
    """emspec_pcm_format: how raw interleaved frames become float32 streams (include/emspec.h, PCM front end)."""
    _fields_ = [("sample_type", C.c_int32), ("channels", C.c_int32), ("views", C.c_int32), ("reserved", C.c_int32),
                ("mix", C.c_float * (PCM_MAX_VIEWS * PCM_MAX_CHANNELS))]
    TYPES = {"s16": PCM_S16, "s24": PCM_S24, "s32": PCM_S32, "f32": PCM_F32}

    @staticmethod
    def view_weights(name, channels):
        """The weights of a named view - the same numbers in every binding: "left" / "right" = channel 0 / 1, "mid" / "side" =
        0.5 (ch0 + ch1) / 0.5 (ch0 - ch1), "mono" = 1 / channels (rounded to binary32) on every channel."""
        w = [0.0] * channels
        if name == "mono":
            return [float(np.float32(1.0) / np.float32(channels))] * channels
        if name == "left":
            w[0] = 1.0
            return w
        if channels < 2:
            raise ValueError(f'view "{name}" needs at least two channels')
        if name == "right":
            w[1] = 1.0
        elif name == "mid":
            w[0], w[1] = 0.5, 0.5
        elif name == "side":
            w[0], w[1] = 0.5, -0.5
        else:
            raise ValueError(f'unknown view "{name}"')
        return w

    @classmethod
    def make(cls, sample_type, channels, views=("mono",)):
        """sample_type: PCM_* or "s16" / "s24" / "s32" / "f32"; views: a list of names ("left", "right", "mid", "side", "mono")
        and / or rows of `channels` weights, or a [views][channels] matrix."""
        f = cls()
        f.sample_type = cls.TYPES.get(sample_type, sample_type) if isinstance(sample_type, str) else int(sample_type)
        f.channels = int(channels)
        rows = [cls.view_weights(v, channels) if isinstance(v, str) else [float(x) for x in v] for v in views]
        if not 1 <= len(rows) <= PCM_MAX_VIEWS or not 1 <= channels <= PCM_MAX_CHANNELS or any(len(r) != channels for r in rows):
            raise ValueError("1..8 views of `channels` (1..8) weights each")
        f.views = len(rows)
        flat = [x for r in rows for x in r]
        for i, x in enumerate(flat):
            f.mix[i] = x
        return f

    @property
    def matrix(self):
        return np.array(self.mix[:self.views * self.channels], np.float32).reshape(self.views, self.channels)

    @property
    def frame_bytes(self):
        return pcm_frame_bytes(self)

    @property
    def dtype(self):
        """numpy dtype of one raw sample (S24: uint8, three per sample)."""
        return {PCM_S16: np.int16, PCM_S24: np.uint8, PCM_S32: np.int32, PCM_F32: np.float32}[self.sample_type]


def pcm_frame_bytes(fmt, diag=False):
    """Bytes per interleaved frame, -1 for an invalid format (emspec_pcm_frame_bytes; no engine, no device)."""
    return int(load(diag).emspec_pcm_frame_bytes(C.byref(fmt) if fmt is not None else None))


def _pcm_rows(src, fmt):
    """src: [sources][frames * samples-per-frame] (or [sources][frames][channels]) array of the format's dtype, C order ->
    (array, sources, frames)."""
    src = np.asarray(src)
    if src.dtype != fmt.dtype or not src.flags.c_contiguous:
        raise EmspecError(ERR_INVALID_ARG, f"raw frames must be a C-contiguous {np.dtype(fmt.dtype).name} array")
    if src.ndim == 1:
        src = src[None]
    sources = src.shape[0]
    row = src.reshape(sources, -1).shape[1] * src.itemsize
    fb = fmt.frame_bytes
    if fb <= 0 or row % fb:
        raise EmspecError(ERR_INVALID_ARG, "invalid format, or a row is not a whole number of frames")
    return src, sources, row // fb


def wire_unpack_host(image, columns, rows, out=None, diag=False):
    """Expand one wire image (numpy uint8) into palette indices [columns, rows] on the host's own cores
    (emspec_wire_unpack_host: plain C, no device, no engine)."""
    image = np.ascontiguousarray(image, np.uint8)
    if out is None:
        out = np.empty((columns, rows), np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size == columns * rows
    lib = load(diag=diag)
    rc = lib.emspec_wire_unpack_host(_np_ptr(image), C.c_int64(image.size), C.c_int64(columns), C.c_int32(rows), _np_ptr(out))
    if rc != 0:
        raise EmspecError(rc, "emspec_wire_unpack_host: the image does not match (columns, rows) or is damaged")
    return out


def peaks_host(db, k, min_db, out=None, diag=False):
    """The k loudest spectral peaks at or above min_db of every column of db [..., rows] float32 on the host's own cores
    (emspec_peaks_host: plain C++, no device, no engine; the definition: include/emspec.h) ->
    float32 [..., k, 2] of (position in row units, dB), loudest first; unused slots (-1, -inf)."""
    db = np.ascontiguousarray(db, np.float32)
    rows = db.shape[-1] if db.ndim else 0
    columns = db.size // rows if rows else 0
    if out is None:
        out = np.empty(db.shape[:-1] + (int(k), 2), np.float32)
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == columns * int(k) * 2
    lib = load(diag=diag)
    rc = lib.emspec_peaks_host(_np_ptr(db), columns, rows, int(k), float(min_db), _np_ptr(out))
    if rc != 0:
        raise EmspecError(rc, lib.emspec_last_error(None).decode())
    return out


def wave_host(pcm, n, hop, factor=1, out=None, diag=False):
    """The waveform envelope of pcm [S, L] (or [L]) float32 on the host's own cores (emspec_wave_host: plain C++, no device, no
    engine; the definition: include/emspec.h) -> float32 [S, Cr, 2] of (lo, hi), Cr = reduced_columns(
    num_columns(L, n, hop), factor): the smallest and the largest sample under each delivered column, with their own bits."""
    pcm = np.ascontiguousarray(pcm, np.float32)
    if pcm.ndim == 1:
        pcm = pcm[None]
    S, L = pcm.shape
    lib = load(diag=diag)
    Cr = max(int(lib.emspec_reduced_columns(max(int(lib.emspec_num_columns(L, n, hop)), 0), factor)), 0)
    if out is None:
        out = np.empty((S, Cr, 2), np.float32)
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == S * Cr * 2
    rc = lib.emspec_wave_host(_np_ptr(pcm), S, L, n, hop, int(factor), _np_ptr(out))
    if rc != 0:
        raise EmspecError(rc, lib.emspec_last_error(None).decode())
    return out


def _level_shape(lib, S, L, n, hop, factor):
    return S, max(int(lib.emspec_reduced_columns(max(int(lib.emspec_num_columns(L, n, hop)), 0), factor)), 0)


def level_host(pcm, n, hop, factor=1, out=None, diag=False):
    """The level records of pcm [S, L] (or [L]) float32 on the host's own cores (emspec_level_host: plain C++, no device, no
    engine; the definition: include/emspec.h) -> LEVEL_DTYPE [S, Cr]: per delivered column the exact sum of
    squares (two limbs), the peak and the odd count of the samples under it, the samples in units of 2^-24."""
    pcm = np.ascontiguousarray(pcm, np.float32)
    if pcm.ndim == 1:
        pcm = pcm[None]
    S, L = pcm.shape
    lib = load(diag=diag)
    if out is None:
        out = np.zeros(_level_shape(lib, S, L, n, hop, factor), LEVEL_DTYPE)
    assert out.dtype == LEVEL_DTYPE and out.flags.c_contiguous
    rc = lib.emspec_level_host(_np_ptr(pcm), S, L, n, hop, int(factor), _np_ptr(out))
    if rc != 0:
        raise EmspecError(rc, lib.emspec_last_error(None).decode())
    return out


def cross_host(pcm, views, a, b, n, hop, factor=1, out=None, diag=False):
    """The cross records of pcm [pairs * views, L] float32 on the host's own cores (emspec_cross_host): pair p's streams are
    p views + a and p views + b -> CROSS_DTYPE [pairs, Cr], the exact sum of the products in two limbs."""
    pcm = np.ascontiguousarray(pcm, np.float32)
    streams, L = pcm.shape
    pairs = streams // views if views > 0 and streams % views == 0 else -1
    lib = load(diag=diag)
    if out is None:
        out = np.zeros(_level_shape(lib, max(pairs, 0), L, n, hop, factor), CROSS_DTYPE)
    assert out.dtype == CROSS_DTYPE and out.flags.c_contiguous
    rc = lib.emspec_cross_host(_np_ptr(pcm), pairs, int(views), int(a), int(b), L, n, hop, int(factor), _np_ptr(out))
    if rc != 0:
        raise EmspecError(rc, lib.emspec_last_error(None).decode())
    return out


def _record(rec, ctype):
    """one record - a numpy structured scalar, a 0-d array or the ctypes structure - as the ctypes structure"""
    return rec if isinstance(rec, ctype) else ctype.from_buffer_copy(np.asarray(rec).tobytes())


def level_window(L, n, hop, factor, g, diag=False):
    """emspec_level_window: the samples in window g (0 where there is none)."""
    return int(load(diag).emspec_level_window(L, n, hop, int(factor), g))


def level_values(level, samples, diag=False):
    """emspec_level_values: (rms_db, peak_db) of one level record over `samples` samples, dB re full scale (|x| = 1); -inf for
    silence."""
    rms, peak = C.c_double(0.0), C.c_double(0.0)
    lv = _record(level, Level)
    if load(diag).emspec_level_values(C.byref(lv), int(samples), C.byref(rms), C.byref(peak)) != OK:
        raise EmspecError(ERR_INVALID_ARG, "level_values needs a record and samples >= 1")
    return rms.value, peak.value


def cross_correlation(level_a, level_b, cross, diag=False):
    """emspec_cross_correlation: rho of a pair's cross record and its two channels' level records, in [-1, 1]; 0 for silence."""
    rho = C.c_double(0.0)
    la, lb, cr = _record(level_a, Level), _record(level_b, Level), _record(cross, Cross)
    if load(diag).emspec_cross_correlation(C.byref(la), C.byref(lb), C.byref(cr), C.byref(rho)) != OK:
        raise EmspecError(ERR_INVALID_ARG, "cross_correlation needs three records")
    return rho.value


def _records_sum(fn, records, dtype, diag):
    records = np.ascontiguousarray(records, dtype).reshape(-1)
    out = np.zeros((), dtype)
    lib = load(diag)
    rc = getattr(lib, fn)(_np_ptr(records) if records.size else None, records.size, _np_ptr(out))
    if rc != OK:
        raise EmspecError(rc, lib.emspec_last_error(None).decode())
    return out


def level_sum(records, diag=False):
    """emspec_level_sum: the field-wise sum (peak: maximum) of one or more LEVEL_DTYPE records - the record of their samples
    together, e.g. a meter's 300 ms of per-hop records of Engine.set_live_level -> a 0-d LEVEL_DTYPE array.  A sum that a limb
    cannot hold, or no record, raises."""
    return _records_sum("emspec_level_sum", records, LEVEL_DTYPE, diag)


def cross_sum(records, diag=False):
    """emspec_cross_sum: as level_sum for CROSS_DTYPE records."""
    return _records_sum("emspec_cross_sum", records, CROSS_DTYPE, diag)


def make_stereo_colormap(brightness=0.5, diag=False):
    """The stereo palette built from make_colormap(brightness): uint8 [33][256][4] for Engine.set_stereo_colormap - row 16 the
    colour map itself, rows towards 0 tinted warm (channel A louder), towards 32 cold (channel B louder)."""
    out = np.empty((STEREO_PAN_LEVELS, 256, 4), np.uint8)
    if load(diag).emspec_make_stereo_colormap(brightness, _np_ptr(out)) != OK:
        raise EmspecError(ERR_INVALID_ARG, "invalid brightness")
    return out


def stereo_host(db, views, a, b, map, palette=None, want=("level", "index", "pan"), diag=False):
    """The stereo image of db [pairs * views, ...] float32 on the host's own cores (emspec_stereo_host: plain C++, no device, no
    engine; the definition: include/emspec.h): pair p's channels are streams p views + a and p views + b ->
    {"level": float32 [pairs, ...], "index": uint8, "pan": uint8, "rgba": uint8 [pairs, ..., 4]}, each present when named in
    `want` ("rgba" needs a palette [33][256][4])."""
    db = np.ascontiguousarray(db, np.float32)
    streams = db.shape[0] if db.ndim else 0
    cells = db.size // streams if streams else 0
    pairs = streams // views if views > 0 and streams % views == 0 else -1
    shape = (max(pairs, 0),) + db.shape[1:]
    out = {"level": np.empty(shape, np.float32) if "level" in want else None,
           "index": np.empty(shape, np.uint8) if "index" in want else None,
           "pan": np.empty(shape, np.uint8) if "pan" in want else None,
           "rgba": np.empty(shape + (4,), np.uint8) if "rgba" in want else None}
    if palette is not None:
        palette = np.ascontiguousarray(palette, np.uint8)
        assert palette.shape == (STEREO_PAN_LEVELS, 256, 4)
    m = _stereo_map(map)
    lib = load(diag=diag)
    rc = lib.emspec_stereo_host(_np_ptr(db), pairs, int(views), int(a), int(b), cells, C.byref(m) if m is not None else None,
                                _np_ptr(palette), _np_ptr(out["level"]), _np_ptr(out["index"]), _np_ptr(out["pan"]), _np_ptr(out["rgba"]))
    if rc != 0:
        raise EmspecError(rc, lib.emspec_last_error(None).decode())
    return out


# the 8-byte records of the overlays, as numpy structured types (include/emspec.h: emspec_peak, emspec_wave)
PEAK_DTYPE = np.dtype([("pos", np.float32), ("db", np.float32)])
WAVE_DTYPE = np.dtype([("lo", np.float32), ("hi", np.float32)])
# ... and the level meters' records (emspec_level: 24 bytes, emspec_cross: 16)
LEVEL_DTYPE = np.dtype([("sq_lo", np.uint64), ("sq_hi", np.uint64), ("peak", np.uint32), ("odd", np.uint32)])
CROSS_DTYPE = np.dtype([("lo", np.uint64), ("hi", np.int64)])


class EmspecError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"emspec error {code}: {msg}")
        self.code = code


_libs = {}


def load(diag=False):
    """Load libemspec.so (or, diag=True, libemspec_diag.so), built in-tree by __graft_entry__.build().
    Raises if absent: there is no fallback."""
    if diag in _libs:
        return _libs[diag]
    path = DIAG_LIB_PATH if diag else LIB_PATH
    # PyTorch ships its own HIP runtime.  If libemspec.so (linked against /opt/rocm's) is loaded first, a later
    # `import torch` brings a second runtime into the process and finds no device ("No HIP GPUs are available"); with
    # torch first, libemspec's libamdhip64 dependency resolves to the copy already loaded.  The Python tooling (tests,
    # bench, smoke) uses torch for device buffers, so settle the order here; hosts without torch are unaffected.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(path)
    lib.emspec_last_error.restype = C.c_char_p
    lib.emspec_last_error.argtypes = [C.c_void_p]
    lib.emspec_device_arch.restype = C.c_char_p
    lib.emspec_device_arch.argtypes = [C.c_void_p]
    lib.emspec_num_columns.restype = C.c_int64
    lib.emspec_num_columns.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    lib.emspec_latency_columns.restype = C.c_int32
    lib.emspec_latency_columns.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.emspec_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
    lib.emspec_destroy.argtypes = [C.c_void_p]
    lib.emspec_destroy.restype = None
    lib.emspec_reset.argtypes = [C.c_void_p]
    lib.emspec_set_colormap.argtypes = [C.c_void_p, C.c_void_p]
    lib.emspec_column.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_int32, C.POINTER(C.c_int64)]
    lib.emspec_column_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
    lib.emspec_push_columns.restype = C.c_int64
    lib.emspec_push_columns.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.emspec_push_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.emspec_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                 C.POINTER(Out)]
    lib.emspec_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emspec_parity_dump.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emspec_parity_dump_device.argtypes = lib.emspec_parity_dump.argtypes + [C.c_void_p]
    lib.emspec_parity_dump_exact.argtypes = lib.emspec_parity_dump.argtypes + [C.c_void_p]
    lib.emspec_uses_fused.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.emspec_set_row_edges_hz.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.emspec_get_row_edges_hz.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.emspec_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    lib.emspec_host_free.argtypes = [C.c_void_p]
    lib.emspec_host_free.restype = None
    lib.emspec_set_display.argtypes = [C.c_void_p, C.c_float, C.c_float]
    lib.emspec_get_tables.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.emspec_comm_unique_id.argtypes = [C.c_void_p]
    lib.emspec_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    lib.emspec_comm_destroy.argtypes = [C.c_void_p]
    lib.emspec_comm_rank.argtypes = [C.c_void_p]
    lib.emspec_comm_world.argtypes = [C.c_void_p]
    lib.emspec_gather_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_uint32,
                                          C.c_void_p, C.POINTER(C.c_int64)]
    lib.emspec_gather_packed_layout.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.emspec_batch_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.emspec_wire_bound.restype = C.c_int64
    lib.emspec_wire_bound.argtypes = [C.c_int64, C.c_int32]
    lib.emspec_wire_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
    lib.emspec_wire_unpack.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    lib.emspec_mode.argtypes = [C.c_void_p]
    lib.emspec_mode.restype = C.c_int32
    lib.emspec_build_info.argtypes = []
    lib.emspec_build_info.restype = C.c_char_p
    lib.emspec_device_status.argtypes = [C.c_void_p]
    lib.emspec_comm_set_timeout.argtypes = [C.c_void_p, C.c_double]
    lib.emspec_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_int32, C.c_void_p]
    lib.emspec_columns_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.emspec_push_columns_multi.restype = C.c_int64
    lib.emspec_push_columns_multi.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.emspec_push_samples_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    lib.emspec_reset_stream.argtypes = [C.c_void_p, C.c_int32]
    lib.emspec_live_streams.argtypes = [C.c_void_p]
    lib.emspec_live_streams.restype = C.c_int32
    lib.emspec_multires_columns.restype = C.c_int64
    lib.emspec_multires_columns.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.emspec_multires_shift.restype = C.c_int32
    lib.emspec_multires_shift.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.emspec_batch_multires.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_int32, C.POINTER(Out)]
    lib.emspec_pcm_frame_bytes.restype = C.c_int64
    lib.emspec_pcm_frame_bytes.argtypes = [C.c_void_p]
    lib.emspec_pcm_decode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    lib.emspec_batch_pcm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                     C.POINTER(Out)]
    lib.emspec_batch_pcm_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_int64, C.c_void_p]
    lib.emspec_push_samples_pcm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    lib.emspec_push_samples_pcm_multires.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                                                     C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                                     C.c_int64, C.c_void_p, C.c_void_p]
    lib.emspec_batch_multires_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if all(hasattr(lib, sym) for sym in OPTIONAL_SYMBOLS):
        lib.emspec_columns_multires.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        lib.emspec_push_columns_multires.restype = C.c_int64
        lib.emspec_push_columns_multires.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        lib.emspec_push_samples_multires.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                                     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                                     C.c_void_p, C.c_void_p]
    if all(hasattr(lib, sym) for sym in REDUCE_SYMBOLS):
        lib.emspec_set_time_reduce.argtypes = [C.c_void_p, C.c_int32]
        lib.emspec_time_reduce.argtypes = [C.c_void_p]
        lib.emspec_time_reduce.restype = C.c_int32
        lib.emspec_reduced_columns.restype = C.c_int64
        lib.emspec_reduced_columns.argtypes = [C.c_int64, C.c_int32]
    if all(hasattr(lib, sym) for sym in PEAKS_SYMBOLS):
        lib.emspec_peaks_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]
        lib.emspec_peaks_host.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p]
        lib.emspec_batch_peaks.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_float, C.c_void_p]
        lib.emspec_batch_peaks_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                                  C.c_int32, C.c_float, C.c_void_p, C.c_void_p]
        lib.emspec_position_hz.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
    if all(hasattr(lib, sym) for sym in WAVE_SYMBOLS):
        lib.emspec_wave_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_void_p]
        lib.emspec_wave_host.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        lib.emspec_set_wave_out.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    if all(hasattr(lib, sym) for sym in MULTIBAND_SYMBOLS):
        lib.emspec_multiband_shifts.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        lib.emspec_multiband_columns.restype = C.c_int64
        lib.emspec_multiband_columns.argtypes = [C.c_int64, C.c_int32, C.c_void_p, C.c_int32]
        lib.emspec_batch_multiband.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_int32, C.c_int32, C.POINTER(Out)]
        lib.emspec_batch_multiband_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                                      C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if all(hasattr(lib, sym) for sym in LIVE_OVERLAY_SYMBOLS):
        lib.emspec_set_live_peaks.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_int64]
        lib.emspec_set_live_wave.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    if all(hasattr(lib, sym) for sym in LIVE_MULTIBAND_SYMBOLS):
        lib.emspec_columns_multiband.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        lib.emspec_push_columns_multiband.restype = C.c_int64
        lib.emspec_push_columns_multiband.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
        lib.emspec_push_samples_multiband.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                                                      C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                                      C.c_void_p, C.c_void_p]
        lib.emspec_push_samples_pcm_multiband.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64,
                                                          C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                                          C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    if all(hasattr(lib, sym) for sym in HISTORY_SYMBOLS):
        lib.emspec_set_live_history.argtypes = [C.c_void_p, C.c_int64]
        lib.emspec_live_history.restype = C.c_int64
        lib.emspec_live_history.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        lib.emspec_history_view_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int64,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.emspec_history_view.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if all(hasattr(lib, sym) for sym in AUDIO_SYMBOLS):
        lib.emspec_set_live_audio.argtypes = [C.c_void_p, C.c_int64]
        lib.emspec_live_audio.restype = C.c_int64
        lib.emspec_live_audio.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        lib.emspec_audio_view_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                                 C.c_int64, C.c_void_p]
        lib.emspec_audio_view.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]
        lib.emspec_audio_batch_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                                                  C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.emspec_audio_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                           C.c_int32, C.POINTER(Out)]
    if all(hasattr(lib, sym) for sym in STEREO_SYMBOLS):
        outs = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.emspec_stereo_default_map.argtypes = [C.c_void_p, C.c_void_p]
        lib.emspec_make_stereo_colormap.argtypes = [C.c_float, C.c_void_p]
        lib.emspec_set_stereo_colormap.argtypes = [C.c_void_p, C.c_void_p]
        lib.emspec_stereo_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                             C.c_void_p] + outs + [C.c_void_p]
        lib.emspec_stereo_host.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p,
                                           C.c_void_p] + outs
        lib.emspec_batch_stereo_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                                   C.c_int32, C.c_int32, C.c_int32, C.c_void_p] + outs + [C.c_void_p]
        lib.emspec_batch_pcm_stereo.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                                C.c_int32, C.c_int32, C.c_int32, C.c_void_p] + outs
        lib.emspec_history_view_stereo_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                          C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_void_p] + outs + [C.c_void_p]
        lib.emspec_history_view_stereo.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                   C.c_int64, C.c_int32, C.c_int64, C.c_void_p] + outs
    if all(hasattr(lib, sym) for sym in LEVEL_SYMBOLS):
        lib.emspec_level_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p]
        lib.emspec_level_host.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        lib.emspec_cross_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        lib.emspec_cross_host.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_void_p]
        lib.emspec_set_level_out.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.emspec_set_cross_out.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]
        lib.emspec_level_window.restype = C.c_int64
        lib.emspec_level_window.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64]
        lib.emspec_level_values.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.emspec_cross_correlation.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if all(hasattr(lib, sym) for sym in LIVE_LEVEL_SYMBOLS):
        lib.emspec_set_live_level.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.emspec_set_live_cross.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]
        lib.emspec_level_sum.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.emspec_cross_sum.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    _libs[diag] = lib
    return lib


def build_info(diag=False):
    """What the loaded library was built from: 'emspec abi=2 sources=<sha16> arch=gfx950' (emspec_build_info)."""
    return load(diag).emspec_build_info().decode()


class PinnedArray:
    """numpy array backed by page-locked host memory from emspec_host_alloc (freed on close/del)."""

    def __init__(self, shape, dtype):
        lib = load()
        self._lib = lib
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        self._ptr = C.c_void_p()
        rc = lib.emspec_host_alloc(n, C.byref(self._ptr))
        if rc != OK:
            raise EmspecError(rc, "emspec_host_alloc failed")
        buf = (C.c_char * n).from_address(self._ptr.value)
        self.array = np.frombuffer(buf, dtype=dt).reshape(shape)

    def close(self):
        if getattr(self, "_ptr", None) is not None and self._ptr.value:
            self.array = None
            self._lib.emspec_host_free(self._ptr)
            self._ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_config(**kw):
    cfg = Config()
    load().emspec_default_config(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


def num_columns(L, n, hop):
    return int(load().emspec_num_columns(L, n, hop))


def reduced_columns(columns, factor, diag=False):
    """Columns a batch call delivers per stream at time reduction `factor`: ceil(columns / factor), -1 for columns < 0 or a
    factor outside 1..65536 (emspec_reduced_columns; no engine, no device)."""
    return int(load(diag).emspec_reduced_columns(columns, factor))


def multires_columns(L, n_low, n_high, hop):
    """Columns of a multi-resolution batch (emspec_multires_columns): num_columns(L, n_low, hop), -1 for a shape
    (n_low, n_high, hop) that is not accepted."""
    return int(load().emspec_multires_columns(L, n_low, n_high, hop))


def multires_shift(n_low, n_high, hop):
    """The high band's column shift (n_low - n_high) / (2 hop) of a multi-resolution batch, -1 for a shape that is not
    accepted (emspec_multires_shift)."""
    return int(load().emspec_multires_shift(n_low, n_high, hop))


def _i32(values):
    """A ctypes int32 array of the values (kept alive by the caller for the length of the call)."""
    values = [int(v) for v in values]
    return (C.c_int32 * max(len(values), 1))(*values)


def multiband_shifts(n, hop):
    """The column shifts (n[0] - n[k]) / (2 hop) of a multi-band batch's bands as a tuple, None for a shape (sizes, hop) that is
    not accepted (emspec_multiband_shifts)."""
    n = list(n)
    out = (C.c_int32 * max(len(n), 1))()
    if load().emspec_multiband_shifts(len(n), _i32(n), hop, out) != 0:
        return None
    return tuple(out[:len(n)])


def multiband_columns(L, n, hop):
    """Columns of a multi-band batch (emspec_multiband_columns): num_columns(L, n[0], hop), -1 for a shape that is not accepted."""
    n = list(n)
    return int(load().emspec_multiband_columns(L, len(n), _i32(n), hop))


def warped_edges_hz(rows, fmin_hz, fmax_hz, low_end_boost=1.0, freq_scale=1.0):
    """rows+1 edges (Hz) of the [BUILD-DEFINED] Frequency Scale / Low-End Boost law, for Engine.set_row_edges_hz."""
    lib = load()
    out = np.empty(rows + 1, np.float32)
    lib.emspec_warped_edges_hz.argtypes = [C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
    if lib.emspec_warped_edges_hz(rows, fmin_hz, fmax_hz, low_end_boost, freq_scale, _np_ptr(out)) != OK:
        raise EmspecError(ERR_INVALID_ARG, "invalid axis parameters")
    return out


def make_colormap(brightness=0.5):
    """The reference ramp scaled by Brightness: uint8 [256][4] for Engine.set_colormap."""
    lib = load()
    out = np.empty((256, 4), np.uint8)
    lib.emspec_make_colormap.argtypes = [C.c_float, C.c_void_p]
    if lib.emspec_make_colormap(brightness, _np_ptr(out)) != OK:
        raise EmspecError(ERR_INVALID_ARG, "invalid brightness")
    return out


def comm_unique_id():
    """128-byte communicator id: rank 0 creates it and hands it to the other ranks (any host channel)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    rc = load().emspec_comm_unique_id(buf)
    if rc != OK:
        raise EmspecError(rc, load().emspec_last_error(None).decode())
    return bytes(buf)


def wire_bound(columns, rows):
    return int(load().emspec_wire_bound(columns, rows))


def latency_columns(n, hop, reassign=True):
    return int(load().emspec_latency_columns(n, hop, int(bool(reassign))))


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


class Engine:
    """One engine = one HIP device + stream (not thread-safe), see emspec.h."""

    def __init__(self, cfg=None, diag=False, **kw):
        self._lib = load(diag)
        self.cfg = cfg if cfg is not None else default_config(**kw)
        h = C.c_void_p()
        rc = self._lib.emspec_create(C.byref(self.cfg), C.byref(h))
        if rc != OK:
            raise EmspecError(rc, self._lib.emspec_last_error(None).decode())
        self._h = h
        self.rows = int(self.cfg.rows)
        # the library must run the mode that was asked for (a version-1 library ignored the field: include/emspec.h)
        if self._lib.emspec_mode(h) != int(self.cfg.mode):
            self._lib.emspec_destroy(h)
            self._h = None
            raise EmspecError(ERR_STATE, "the library did not honour the requested arithmetic mode")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.emspec_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != OK:
            raise EmspecError(rc, self._lib.emspec_last_error(self._h).decode())

    @property
    def mode(self):
        return int(self._lib.emspec_mode(self._h))

    def device_status(self):
        """Synchronise the device and raise if a kernel flagged a protocol error (emspec_device_status)."""
        self._chk(self._lib.emspec_device_status(self._h))

    @property
    def arch(self):
        return self._lib.emspec_device_arch(self._h).decode()

    def fused(self, n, hop, reassign=True):
        return bool(self._lib.emspec_uses_fused(self._h, n, hop, int(bool(reassign))))

    def set_colormap(self, lut):
        lut = np.ascontiguousarray(lut, np.uint8)
        assert lut.shape == (256, 4)
        self._chk(self._lib.emspec_set_colormap(self._h, _np_ptr(lut)))

    def set_display(self, smoothing=0.0, agc_strength=0.0):
        """Temporal smoothing in [0,0.95] and adaptive-brightness strength in [0,1]; (0,0) = off."""
        self._chk(self._lib.emspec_set_display(self._h, smoothing, agc_strength))

    def set_time_reduce(self, factor):
        """Time reduction of the batch entries (emspec_set_time_reduce): groups of `factor` finished columns
        collapse into one by maximum, every batch call returns reduced_columns(C, factor) columns per stream.  1 = off."""
        self._chk(self._lib.emspec_set_time_reduce(self._h, int(factor)))

    @property
    def time_reduce(self):
        return int(self._lib.emspec_time_reduce(self._h)) if hasattr(self._lib, "emspec_time_reduce") else 1

    def out_columns(self, columns):
        """Columns per stream a batch call delivers for `columns` full-rate ones at the engine's time reduction."""
        f = self.time_reduce
        return columns if f == 1 else reduced_columns(columns, f)

    def set_row_edges_hz(self, edges_hz):
        """rows+1 strictly increasing edges in Hz, or None for the configured log axis."""
        if edges_hz is None:
            self._chk(self._lib.emspec_set_row_edges_hz(self._h, None, 0))
        else:
            edges_hz = np.ascontiguousarray(edges_hz, np.float32)
            self._chk(self._lib.emspec_set_row_edges_hz(self._h, _np_ptr(edges_hz), edges_hz.size))

    def row_edges_hz(self):
        out = np.empty(self.rows + 1, np.float32)
        self._chk(self._lib.emspec_get_row_edges_hz(self._h, _np_ptr(out), out.size))
        return out

    def tables(self, n):
        eb = np.empty(self.rows + 1, np.float32)
        tw = np.empty(n, np.float32)
        self._chk(self._lib.emspec_get_tables(self._h, n, _np_ptr(eb), _np_ptr(tw)))
        return tw, eb

    # -- batch, host buffers ------------------------------------------------
    def batch(self, pcm, n, hop, reassign=True, want=("db",), db_out=None):
        pcm = np.ascontiguousarray(pcm, np.float32)
        if pcm.ndim == 1:
            pcm = pcm[None]
        S, L = pcm.shape
        Cn = self.out_columns(num_columns(L, n, hop))
        db = (db_out if db_out is not None else np.empty((S, Cn, self.rows), np.float32)) if "db" in want else None
        assert db is None or (db.shape == (S, Cn, self.rows) and db.dtype == np.float32 and db.flags.c_contiguous)
        rgba = np.empty((S, Cn, self.rows, 4), np.uint8) if "rgba" in want else None
        idx = np.empty((S, Cn, self.rows), np.uint8) if "index" in want else None
        out = Out(_np_ptr(db), _np_ptr(rgba), _np_ptr(idx))
        self._chk(self._lib.emspec_batch(self._h, _np_ptr(pcm), S, L, n, hop, int(bool(reassign)), C.byref(out)))
        return {"db": db, "rgba": rgba, "index": idx}

    def batch_packed(self, pcm, n, hop, reassign=True, wire=None):
        """Host buffers in, the palette-index columns out as ONE lossless wire image per stream (emspec_batch_packed):
        returns (wire uint8 array, offsets int64 [S+1]); stream s is wire[offsets[s]:offsets[s+1]], expand it with
        wire_unpack_host(image, columns, rows).  `wire`: optional preallocated (pinned) uint8 array."""
        pcm = np.ascontiguousarray(pcm, np.float32)
        if pcm.ndim == 1:
            pcm = pcm[None]
        S, L = pcm.shape
        Cn = self.out_columns(num_columns(L, n, hop))
        if wire is None:
            wire = np.empty(S * wire_bound(Cn, self.rows), np.uint8)
        offsets = np.zeros(S + 1, np.int64)
        self._chk(self._lib.emspec_batch_packed(self._h, _np_ptr(pcm), S, L, n, hop, int(bool(reassign)), _np_ptr(wire),
                                                C.c_int64(wire.size), offsets.ctypes.data_as(C.c_void_p)))
        return wire, offsets

    # -- PCM front end: raw interleaved frames in (include/emspec.h) ---------------------------------
    def pcm_decode_device(self, src_t, fmt, sources, frames, src_stride_bytes=None, offset_bytes=0, out=None, stream=None):
        """The decode kernel by itself (emspec_pcm_decode_device).  src_t: a CUDA tensor holding the raw bytes (any dtype);
        source i starts offset_bytes + i * src_stride_bytes into it.  Returns the float32 CUDA tensor [sources * views][frames];
        enqueued on `stream` (default: the current torch stream), not synchronised."""
        import torch
        assert src_t.is_cuda and src_t.is_contiguous()
        fb = fmt.frame_bytes
        if src_stride_bytes is None:
            src_stride_bytes = frames * max(fb, 0)
        assert fb <= 0 or sources == 0 or offset_bytes + (sources - 1) * src_stride_bytes + frames * fb <= src_t.numel() * src_t.element_size()
        if out is None:
            out = torch.empty((sources * max(fmt.views, 0), frames), dtype=torch.float32, device=src_t.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
        st = stream if stream is not None else torch.cuda.current_stream(src_t.device)
        self._chk(self._lib.emspec_pcm_decode_device(self._h, C.c_void_p(src_t.data_ptr() + offset_bytes), C.byref(fmt), sources,
                                                     frames, src_stride_bytes, C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream)))
        return out

    def batch_pcm(self, src, fmt, n, hop, reassign=True, want=("db",)):
        """emspec_batch from raw frames: src [sources][frames x channels] of fmt.dtype (S24: uint8, 3 per sample) ->
        {"db", "rgba", "index"} laid out [sources * views][columns][rows]."""
        src, sources, frames = _pcm_rows(src, fmt)
        S, Cn = sources * fmt.views, self.out_columns(num_columns(frames, n, hop))
        db = np.empty((S, Cn, self.rows), np.float32) if "db" in want else None
        rgba = np.empty((S, Cn, self.rows, 4), np.uint8) if "rgba" in want else None
        idx = np.empty((S, Cn, self.rows), np.uint8) if "index" in want else None
        out = Out(_np_ptr(db), _np_ptr(rgba), _np_ptr(idx))
        self._chk(self._lib.emspec_batch_pcm(self._h, _np_ptr(src), C.byref(fmt), sources, frames, n, hop, int(bool(reassign)),
                                             C.byref(out)))
        return {"db": db, "rgba": rgba, "index": idx}

    def batch_pcm_packed(self, src, fmt, n, hop, reassign=True, wire=None):
        """emspec_batch_packed from raw frames: (wire uint8 array, offsets int64 [sources * views + 1]), as batch_packed."""
        src, sources, frames = _pcm_rows(src, fmt)
        S, Cn = sources * fmt.views, self.out_columns(num_columns(frames, n, hop))
        if wire is None:
            wire = np.empty(S * wire_bound(Cn, self.rows), np.uint8)
        offsets = np.zeros(S + 1, np.int64)
        self._chk(self._lib.emspec_batch_pcm_packed(self._h, _np_ptr(src), C.byref(fmt), sources, frames, n, hop, int(bool(reassign)),
                                                    _np_ptr(wire), C.c_int64(wire.size), offsets.ctypes.data_as(C.c_void_p)))
        return wire, offsets

    def push_samples_pcm(self, block, fmt, n, hop, reassign=True, n_high=0, split_row=0, want_db=True, want_rgba=False, db=None,
                         rgba=None, count=None, offset=0, max_columns=None, split_rows=None):
        """Live session from raw frames (emspec_push_samples_pcm; n_high != 0: emspec_push_samples_pcm_multires with n = n_low;
        n a sequence of sizes and split_rows given: emspec_push_samples_pcm_multiband).
        block [sources][frames x channels] of fmt.dtype; the window of `count` frames from frame `offset` of every row is fed
        -> (db [sources * views][k][rows], rgba, counts, first_columns) as push_samples_multi."""
        block, sources, width = _pcm_rows(block, fmt)
        fb = fmt.frame_bytes
        if count is None:
            count = width - offset
        assert 0 <= offset and offset + count <= width
        S = sources * fmt.views
        bands = not isinstance(n, (int, np.integer))
        if bands:
            K, sizes, splits = self._bands(n, split_rows)
            k = self.push_columns_multiband(count, n, hop, reassign)
        else:
            k = self.push_columns_multires(count, n, n_high, hop, reassign) if n_high else self.push_columns_multi(count, n, hop, reassign)
        if k < 0:   # (the call itself names the rule the shape breaks)
            k = 0
        if db is not None:
            k = db.shape[1]
        elif rgba is not None:
            k = rgba.shape[1]
        db, rgba = self._live_out(S, k, want_db, want_rgba, db, rgba)
        counts, firsts = np.empty(S, np.int64), np.empty(S, np.int64)
        base = C.c_void_p(block.ctypes.data + fb * offset)
        cap = k if max_columns is None else max_columns
        if bands:
            rc = self._lib.emspec_push_samples_pcm_multiband(self._h, base, C.byref(fmt), sources, count, width * fb, K, sizes,
                                                             splits, hop, int(bool(reassign)),
                                                             _np_ptr(db), _np_ptr(rgba), self.rows, cap, _np_ptr(counts),
                                                             _np_ptr(firsts))
        elif n_high:
            rc = self._lib.emspec_push_samples_pcm_multires(self._h, base, C.byref(fmt), sources, count, width * fb, n, n_high, hop,
                                                            split_row, int(bool(reassign)), _np_ptr(db), _np_ptr(rgba), self.rows,
                                                            cap, _np_ptr(counts), _np_ptr(firsts))
        else:
            rc = self._lib.emspec_push_samples_pcm(self._h, base, C.byref(fmt), sources, count, width * fb, n, hop,
                                                   int(bool(reassign)), _np_ptr(db), _np_ptr(rgba), self.rows, cap,
                                                   _np_ptr(counts), _np_ptr(firsts))
        self._chk(rc)
        return db, rgba, counts, firsts

    # -- batch, device-resident torch tensors ---------------------------------
    def batch_device(self, pcm_t, n, hop, reassign=True, db=None, rgba=None, index=None, stream=None):
        """pcm_t: contiguous float32 CUDA tensor [S, L]; outputs: preallocated CUDA tensors or None.
        Enqueues on `stream` (a torch.cuda.Stream; default: the current torch stream); does not synchronise."""
        import torch
        assert pcm_t.is_cuda and pcm_t.dtype == torch.float32 and pcm_t.is_contiguous() and pcm_t.dim() == 2
        S, L = pcm_t.shape
        st = stream if stream is not None else torch.cuda.current_stream(pcm_t.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        for t in (db, rgba, index):
            assert t is None or (t.is_cuda and t.is_contiguous())
        self._chk(self._lib.emspec_batch_device(self._h, ptr(pcm_t), S, L, n, hop, int(bool(reassign)), ptr(db),
                                                ptr(rgba), ptr(index), C.c_void_p(st.cuda_stream)))

    # -- spectral peaks: (position in row units, dB) pairs, float32 [..., k, 2] -----------------------
    def peaks_device(self, db_t, k, min_db, out=None, stream=None):
        """emspec_peaks_device: db_t a contiguous float32 CUDA tensor [..., rows] (any rows % 4 == 0 in 4 .. 4096) ->
        CUDA tensor [..., k, 2], the k loudest peaks at or above min_db of every column.  Enqueues; does not synchronise."""
        import torch
        assert db_t.is_cuda and db_t.dtype == torch.float32 and db_t.is_contiguous() and db_t.dim() >= 1
        rows = db_t.shape[-1]
        columns = db_t.numel() // rows if rows else 0
        if out is None:
            out = torch.empty(tuple(db_t.shape[:-1]) + (int(k), 2), dtype=torch.float32, device=db_t.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == columns * int(k) * 2
        st = stream if stream is not None else torch.cuda.current_stream(db_t.device)
        self._chk(self._lib.emspec_peaks_device(self._h, C.c_void_p(db_t.data_ptr()), columns, rows, int(k), float(min_db),
                                                C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream)))
        return out

    def batch_peaks_device(self, pcm_t, n, hop, reassign=True, k=8, min_db=-60.0, out=None, stream=None):
        """emspec_batch_peaks_device: pcm_t a contiguous float32 CUDA tensor [S, L] -> CUDA tensor [S, columns, k, 2]: the
        peaks of the dB batch_device would deliver.  Enqueues; does not synchronise."""
        import torch
        assert pcm_t.is_cuda and pcm_t.dtype == torch.float32 and pcm_t.is_contiguous() and pcm_t.dim() == 2
        S, L = pcm_t.shape
        Cn = num_columns(L, n, hop)
        if out is None:
            out = torch.empty((S, Cn, int(k), 2), dtype=torch.float32, device=pcm_t.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == S * Cn * int(k) * 2
        st = stream if stream is not None else torch.cuda.current_stream(pcm_t.device)
        self._chk(self._lib.emspec_batch_peaks_device(self._h, C.c_void_p(pcm_t.data_ptr()), S, L, n, hop, int(bool(reassign)),
                                                      int(k), float(min_db), C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream)))
        return out

    def batch_peaks(self, pcm, n, hop, reassign=True, k=8, min_db=-60.0, out=None):
        """emspec_batch_peaks: host samples [S, L] in, float32 [S, columns, k, 2] out (pageable, or a PinnedArray's array):
        the pipeline of batch(), but only the peak lists cross PCIe on the way out."""
        pcm = np.ascontiguousarray(pcm, np.float32)
        if pcm.ndim == 1:
            pcm = pcm[None]
        S, L = pcm.shape
        Cn = num_columns(L, n, hop)
        if out is None:
            out = np.empty((S, Cn, int(k), 2), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == S * Cn * int(k) * 2
        self._chk(self._lib.emspec_batch_peaks(self._h, _np_ptr(pcm), S, L, n, hop, int(bool(reassign)), int(k), float(min_db),
                                               _np_ptr(out)))
        return out

    def position_hz(self, pos):
        """emspec_position_hz: a peak's position in row units -> Hz on the engine's row axis (log-interpolated inside the row)."""
        hz = C.c_double(0.0)
        self._chk(self._lib.emspec_position_hz(self._h, float(pos), C.byref(hz)))
        return hz.value

    # -- waveform envelope: (lo, hi) pairs of the samples under each delivered column, float32 [..., 2] ----
    def wave_device(self, pcm_t, n, hop, factor=1, out=None, stream=None):
        """emspec_wave_device: pcm_t a contiguous float32 CUDA tensor [S, L] (4-byte aligned) -> CUDA tensor [S, Cr, 2],
        Cr = reduced_columns(num_columns(L, n, hop), factor).  `factor` is the call's own: the engine's time reduction plays no
        part.  Enqueues; does not synchronise."""
        import torch
        assert pcm_t.is_cuda and pcm_t.dtype == torch.float32 and pcm_t.is_contiguous() and pcm_t.dim() == 2
        S, L = pcm_t.shape
        Cr = max(reduced_columns(max(num_columns(L, n, hop), 0), factor), 0)
        if out is None:
            out = torch.empty((S, Cr, 2), dtype=torch.float32, device=pcm_t.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == S * Cr * 2
        st = stream if stream is not None else torch.cuda.current_stream(pcm_t.device)
        self._chk(self._lib.emspec_wave_device(self._h, C.c_void_p(pcm_t.data_ptr()), S, L, n, hop, int(factor),
                                               C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream)))
        return out

    def set_wave_out(self, wave):
        """emspec_set_wave_out: while set, batch(), batch_packed(), batch_pcm(), batch_pcm_packed(), batch_multires(), batch_multiband() and
        batch_peaks() also write the envelope of their streams to `wave`, a C-contiguous float32 numpy array of
        streams x delivered columns x 2 values or more (pageable, or a PinnedArray's array); None clears it.  The engine keeps a
        reference to the array while it is set."""
        if wave is None:
            self._chk(self._lib.emspec_set_wave_out(self._h, None, 0))
            self._wave_out = None
            return
        assert isinstance(wave, np.ndarray) and wave.dtype == np.float32 and wave.flags.c_contiguous and wave.flags.writeable
        self._chk(self._lib.emspec_set_wave_out(self._h, _np_ptr(wave), wave.size // 2))
        self._wave_out = wave

    # -- level meters: exact sums of squares / products of the samples under each delivered column ----------
    def level_device(self, pcm_t, n, hop, factor=1, out=None, stream=None):
        """emspec_level_device: pcm_t a contiguous float32 CUDA tensor [S, L] (4-byte aligned) -> uint8 CUDA tensor
        [S, Cr, 24] of emspec_level records (8-byte aligned; .cpu().numpy().view(LEVEL_DTYPE)[..., 0] names the fields).
        `factor` is the call's own.  Enqueues; does not synchronise."""
        import torch
        assert pcm_t.is_cuda and pcm_t.dtype == torch.float32 and pcm_t.is_contiguous() and pcm_t.dim() == 2
        S, L = pcm_t.shape
        Cr = max(reduced_columns(max(num_columns(L, n, hop), 0), factor), 0)
        if out is None:
            out = torch.empty((S, Cr, 24), dtype=torch.uint8, device=pcm_t.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == S * Cr * 24
        st = stream if stream is not None else torch.cuda.current_stream(pcm_t.device)
        self._chk(self._lib.emspec_level_device(self._h, C.c_void_p(pcm_t.data_ptr()), S, L, n, hop, int(factor),
                                                C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream)))
        return out

    def cross_device(self, pcm_t, views, a, b, n, hop, factor=1, out=None, stream=None):
        """emspec_cross_device: pcm_t [pairs * views, L] as for level_device; pair p's streams are p views + a and p views + b
        -> uint8 CUDA tensor [pairs, Cr, 16] of emspec_cross records (view as CROSS_DTYPE).  Enqueues; does not synchronise."""
        import torch
        assert pcm_t.is_cuda and pcm_t.dtype == torch.float32 and pcm_t.is_contiguous() and pcm_t.dim() == 2
        streams, L = pcm_t.shape
        pairs = streams // views if views > 0 and streams % views == 0 else -1
        Cr = max(reduced_columns(max(num_columns(L, n, hop), 0), factor), 0)
        if out is None:
            out = torch.empty((max(pairs, 0), Cr, 16), dtype=torch.uint8, device=pcm_t.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == max(pairs, 0) * Cr * 16
        st = stream if stream is not None else torch.cuda.current_stream(pcm_t.device)
        self._chk(self._lib.emspec_cross_device(self._h, C.c_void_p(pcm_t.data_ptr()), pairs, int(views), int(a), int(b), L, n, hop,
                                                int(factor), C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream)))
        return out

    def set_level_out(self, level):
        """emspec_set_level_out: while set, every call that honours set_wave_out also writes the level records of its streams to
        `level`, a C-contiguous numpy array of LEVEL_DTYPE with streams x delivered columns records or more; None clears it.
        The engine keeps a reference to the array while it is set."""
        if level is None:
            self._chk(self._lib.emspec_set_level_out(self._h, None, 0))
            self._level_out = None
            return
        assert isinstance(level, np.ndarray) and level.dtype == LEVEL_DTYPE and level.flags.c_contiguous and level.flags.writeable
        self._chk(self._lib.emspec_set_level_out(self._h, _np_ptr(level), level.size))
        self._level_out = level

    def set_cross_out(self, a, b, cross):
        """emspec_set_cross_out: while set, batch_pcm(), batch_pcm_packed() and batch_pcm_stereo() also write the cross records
        of views a and b of each source to `cross`, a C-contiguous numpy array of CROSS_DTYPE with sources x delivered columns
        records or more; None clears it.  The float-stream host calls raise ERR_STATE while it is set."""
        if cross is None:
            self._chk(self._lib.emspec_set_cross_out(self._h, 0, 0, None, 0))
            self._cross_out = None
            return
        assert isinstance(cross, np.ndarray) and cross.dtype == CROSS_DTYPE and cross.flags.c_contiguous and cross.flags.writeable
        self._chk(self._lib.emspec_set_cross_out(self._h, int(a), int(b), _np_ptr(cross), cross.size))
        self._cross_out = cross

    # -- multi-resolution batch: n_low below split_row, n_high from it up, one column grid --------
    def split_row_for_hz(self, hz):
        """The smallest admissible split_row (a multiple of 4 in [64, rows - 64]) whose lower edge is >= hz."""
        edges = self.row_edges_hz()
        for r in range(64, self.rows - 63, 4):
            if edges[r] >= np.float32(hz):
                return r
        raise EmspecError(ERR_INVALID_ARG, f"no admissible split row at or above {hz} Hz")

    def batch_multires(self, pcm, n_low, n_high, hop, split_row, reassign=True, want=("db",)):
        """Host buffers in and out (emspec_batch_multires): [S][C][rows] outputs as in batch(), C = multires_columns."""
        pcm = np.ascontiguousarray(pcm, np.float32)
        if pcm.ndim == 1:
            pcm = pcm[None]
        S, L = pcm.shape
        Cn = self.out_columns(max(multires_columns(L, n_low, n_high, hop), 0))
        db = np.empty((S, Cn, self.rows), np.float32) if "db" in want else None
        rgba = np.empty((S, Cn, self.rows, 4), np.uint8) if "rgba" in want else None
        idx = np.empty((S, Cn, self.rows), np.uint8) if "index" in want else None
        out = Out(_np_ptr(db), _np_ptr(rgba), _np_ptr(idx))
        self._chk(self._lib.emspec_batch_multires(self._h, _np_ptr(pcm), S, L, n_low, n_high, hop, split_row,
                                                  int(bool(reassign)), C.byref(out)))
        return {"db": db, "rgba": rgba, "index": idx}

    def batch_multires_device(self, pcm_t, n_low, n_high, hop, split_row, reassign=True, db=None, rgba=None, index=None,
                              stream=None):
        """Device-resident torch tensors (emspec_batch_multires_device), as batch_device(); does not synchronise."""
        import torch
        assert pcm_t.is_cuda and pcm_t.dtype == torch.float32 and pcm_t.is_contiguous() and pcm_t.dim() == 2
        S, L = pcm_t.shape
        st = stream if stream is not None else torch.cuda.current_stream(pcm_t.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        for t in (db, rgba, index):
            assert t is None or (t.is_cuda and t.is_contiguous())
        self._chk(self._lib.emspec_batch_multires_device(self._h, ptr(pcm_t), S, L, n_low, n_high, hop, split_row,
                                                         int(bool(reassign)), ptr(db), ptr(rgba), ptr(index),
                                                         C.c_void_p(st.cuda_stream)))

    # -- multi-band batch: up to four FFT sizes n[0] > n[1] > ..., band k from split_rows[k - 1] up ---------
    def batch_multiband(self, pcm, n, split_rows, hop, reassign=True, want=("db",)):
        """Host buffers in and out (emspec_batch_multiband): [S][C][rows] outputs as in batch(), C = multiband_columns."""
        pcm = np.ascontiguousarray(pcm, np.float32)
        if pcm.ndim == 1:
            pcm = pcm[None]
        S, L = pcm.shape
        n, split_rows = list(n), list(split_rows)
        Cn = self.out_columns(max(multiband_columns(L, n, hop), 0))
        db = np.empty((S, Cn, self.rows), np.float32) if "db" in want else None
        rgba = np.empty((S, Cn, self.rows, 4), np.uint8) if "rgba" in want else None
        idx = np.empty((S, Cn, self.rows), np.uint8) if "index" in want else None
        out = Out(_np_ptr(db), _np_ptr(rgba), _np_ptr(idx))
        self._chk(self._lib.emspec_batch_multiband(self._h, _np_ptr(pcm), S, L, len(n), _i32(n), _i32(split_rows), hop,
                                                   int(bool(reassign)), C.byref(out)))
        return {"db": db, "rgba": rgba, "index": idx}

    def batch_multiband_device(self, pcm_t, n, split_rows, hop, reassign=True, db=None, rgba=None, index=None, stream=None):
        """Device-resident torch tensors (emspec_batch_multiband_device), as batch_device(); does not synchronise."""
        import torch
        assert pcm_t.is_cuda and pcm_t.dtype == torch.float32 and pcm_t.is_contiguous() and pcm_t.dim() == 2
        S, L = pcm_t.shape
        n, split_rows = list(n), list(split_rows)
        st = stream if stream is not None else torch.cuda.current_stream(pcm_t.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        for t in (db, rgba, index):
            assert t is None or (t.is_cuda and t.is_contiguous())
        self._chk(self._lib.emspec_batch_multiband_device(self._h, ptr(pcm_t), S, L, len(n), _i32(n), _i32(split_rows), hop,
                                                          int(bool(reassign)), ptr(db), ptr(rgba), ptr(index),
                                                          C.c_void_p(st.cuda_stream)))

    # -- multi-GPU: RCCL communicator + gather of finished palette-index columns ----
    def comm_init(self, comm_id, rank, world):
        """Collective over all `world` ranks (one engine / process per GPU); comm_id from comm_unique_id() of rank 0."""
        assert len(comm_id) == COMM_ID_BYTES
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(comm_id)
        self._chk(self._lib.emspec_comm_init(self._h, buf, rank, world))

    def comm_destroy(self):
        self._chk(self._lib.emspec_comm_destroy(self._h))

    def comm_set_timeout(self, seconds):
        """Bound on the host wait inside gather_columns (the size exchange); 0 = none.  On expiry the communicator is aborted."""
        self._chk(self._lib.emspec_comm_set_timeout(self._h, float(seconds)))

    @property
    def comm_rank(self):
        return int(self._lib.emspec_comm_rank(self._h))

    @property
    def comm_world(self):
        return int(self._lib.emspec_comm_world(self._h))

    def gather_columns(self, index_t, root=0, out=None, stream=None, loopback=False, packed=False):
        """packed=True: the root keeps the ranks' wire images packed in `out` (directory + images; expand on demand with
        wire_unpack at gather_packed_layout(rank)); capacity 256*(world+1) + sum of wire_bound over the ranks.
        index_t: contiguous uint8 CUDA tensor [..., rows] of this rank's finished columns; out (root only):
        uint8 CUDA tensor holding the ranks' blocks in rank order ([world, ...same shape...] when the shards are equal;
        the library checks that the announced shards fit).  Returns the bytes this rank put on the wire."""
        import torch
        assert index_t.is_cuda and index_t.dtype == torch.uint8 and index_t.is_contiguous() and index_t.shape[-1] == self.rows
        columns = index_t.numel() // self.rows
        st = stream if stream is not None else torch.cuda.current_stream(index_t.device)
        if out is not None:
            assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
        sent = C.c_int64(0)
        self._chk(self._lib.emspec_gather_columns(self._h, C.c_void_p(index_t.data_ptr()), columns, root,
                                                  C.c_void_p(out.data_ptr()) if out is not None else None,
                                                  out.numel() if out is not None else 0,
                                                  (GATHER_LOOPBACK if loopback else 0) | (GATHER_PACKED if packed else 0),
                                                  C.c_void_p(st.cuda_stream), C.byref(sent)))
        return int(sent.value)

    def gather_packed_layout(self, rank):
        """Root, after gather_columns(packed=True): (offset in the gathered buffer, image bytes, columns) of `rank`'s image."""
        off, nb, cols = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._lib.emspec_gather_packed_layout(self._h, rank, C.byref(off), C.byref(nb), C.byref(cols)))
        return int(off.value), int(nb.value), int(cols.value)

    def batch_gather(self, pcm, n, hop, reassign=True, root=0, want_db=False):
        """Host buffers: this rank's streams -> (gathered index [world,S,C,rows] on root else None, own dB or None, wire bytes)."""
        pcm = np.ascontiguousarray(pcm, np.float32)
        S, L = pcm.shape
        Cn = self.out_columns(num_columns(L, n, hop))
        allidx = np.empty((self.comm_world, S, Cn, self.rows), np.uint8) if self.comm_rank == root else None
        db = np.empty((S, Cn, self.rows), np.float32) if want_db else None
        sent = C.c_int64(0)
        self._chk(self._lib.emspec_batch_gather(self._h, _np_ptr(pcm), S, L, n, hop, int(bool(reassign)), root, _np_ptr(allidx),
                                                _np_ptr(db), C.byref(sent)))
        return allidx, db, int(sent.value)

    def wire_pack(self, index_t, wire_t, stream=None, want_size=True):
        """index_t uint8 CUDA [columns, rows] -> wire_t (uint8 CUDA, >= wire_bound bytes); returns the image size."""
        import torch
        columns = index_t.numel() // self.rows
        assert wire_t.numel() >= wire_bound(columns, self.rows)
        st = stream if stream is not None else torch.cuda.current_stream(index_t.device)
        n = C.c_int64(-1)
        self._chk(self._lib.emspec_wire_pack(self._h, C.c_void_p(index_t.data_ptr()), columns, C.c_void_p(wire_t.data_ptr()),
                                             C.byref(n) if want_size else None, C.c_void_p(st.cuda_stream)))
        return int(n.value)

    def wire_unpack(self, wire_t, wire_bytes, out_t, stream=None):
        import torch
        columns = out_t.numel() // self.rows
        st = stream if stream is not None else torch.cuda.current_stream(out_t.device)
        self._chk(self._lib.emspec_wire_unpack(self._h, C.c_void_p(wire_t.data_ptr()), wire_bytes, columns,
                                               C.c_void_p(out_t.data_ptr()), C.c_void_p(st.cuda_stream)))

    # -- parity dump ------------------------------------------------------------
    def parity_dump(self, pcm, n, hop, reassign=True, frame0=0, nframes=None):
        pcm = np.ascontiguousarray(pcm, np.float32)
        if pcm.ndim == 1:
            pcm = pcm[None]
        S, L = pcm.shape
        if nframes is None:
            nframes = num_columns(L, n, hop) - frame0
        K = n // 2 + 1
        pw = np.empty((S, nframes, K), np.float32)
        col = np.empty((S, nframes, K), np.int32)
        row = np.empty((S, nframes, K), np.int32)
        self._chk(self._lib.emspec_parity_dump(self._h, _np_ptr(pcm), S, L, n, hop, int(bool(reassign)), frame0,
                                               nframes, _np_ptr(pw), _np_ptr(col), _np_ptr(row)))
        return pw, col, row

    def parity_dump_device(self, pcm_t, n, hop, reassign=True, frame0=0, nframes=None, power=None, col=None, row=None, stream=None):
        """emspec_parity_dump_device: pcm_t a contiguous float32 CUDA tensor [S, L] -> (power float32, col int32, row int32)
        CUDA tensors [S, nframes, n/2+1] (those given are written in place).  FAST-mode engines only.  Enqueues on `stream`
        (default: the current torch stream); does not synchronise."""
        import torch
        assert pcm_t.is_cuda and pcm_t.dtype == torch.float32 and pcm_t.is_contiguous() and pcm_t.dim() == 2
        S, L = pcm_t.shape
        if nframes is None:
            nframes = num_columns(L, n, hop) - frame0
        shape = (S, max(int(nframes), 0), n // 2 + 1)
        power = torch.empty(shape, dtype=torch.float32, device=pcm_t.device) if power is None else power
        col = torch.empty(shape, dtype=torch.int32, device=pcm_t.device) if col is None else col
        row = torch.empty(shape, dtype=torch.int32, device=pcm_t.device) if row is None else row
        for t, dt in ((power, torch.float32), (col, torch.int32), (row, torch.int32)):
            assert t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape
        st = stream if stream is not None else torch.cuda.current_stream(pcm_t.device)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        self._chk(self._lib.emspec_parity_dump_device(self._h, ptr(pcm_t), S, L, n, hop, int(bool(reassign)), frame0, nframes,
                                                      ptr(power), ptr(col), ptr(row), C.c_void_p(st.cuda_stream)))
        return power, col, row

    def parity_dump_exact(self, pcm, n, hop, reassign=True, frame0=0, nframes=None):
        """EXACT-mode engine: (power float64, col, row, q int64), each [S][nframes][n/2+1]."""
        pcm = np.ascontiguousarray(pcm, np.float32)
        if pcm.ndim == 1:
            pcm = pcm[None]
        S, L = pcm.shape
        if nframes is None:
            nframes = num_columns(L, n, hop) - frame0
        K = n // 2 + 1
        pw = np.empty((S, nframes, K), np.float64)
        col = np.empty((S, nframes, K), np.int32)
        row = np.empty((S, nframes, K), np.int32)
        q = np.empty((S, nframes, K), np.int64)
        self._chk(self._lib.emspec_parity_dump_exact(self._h, _np_ptr(pcm), S, L, n, hop, int(bool(reassign)), frame0,
                                                     nframes, _np_ptr(pw), _np_ptr(col), _np_ptr(row), _np_ptr(q)))
        return pw, col, row, q

    # -- streaming: the renderer's computeSpectrogramColumn -------------------------
    def column(self, frame, hop, reassign=True, want_rgba=False):
        frame = np.ascontiguousarray(frame, np.float32)
        n = frame.size
        db = np.empty(self.rows, np.float32)
        rgba = np.empty((self.rows, 4), np.uint8) if want_rgba else None
        c = C.c_int64(-2)
        self._chk(self._lib.emspec_column(self._h, _np_ptr(frame), n, hop, int(bool(reassign)), _np_ptr(db),
                                          _np_ptr(rgba), self.rows, C.byref(c)))
        return (db, rgba, int(c.value)) if want_rgba else (db, int(c.value))

    def push_samples(self, samples, n, hop, reassign=True, want_rgba=False):
        """Feed a block of samples of any length; returns (db [k][rows], first_column) (+ rgba) for the k columns
        the block completed (k may be 0)."""
        samples = np.ascontiguousarray(samples, np.float32).reshape(-1)
        k = int(self._lib.emspec_push_columns(self._h, samples.size, n, hop, int(bool(reassign))))
        if k < 0:
            raise EmspecError(ERR_INVALID_ARG, "invalid fft size / hop")
        db = np.empty((k, self.rows), np.float32)
        rgba = np.empty((k, self.rows, 4), np.uint8) if want_rgba else None
        cnt, first = C.c_int64(-1), C.c_int64(-2)
        self._chk(self._lib.emspec_push_samples(self._h, _np_ptr(samples), samples.size, n, hop, int(bool(reassign)),
                                                _np_ptr(db), _np_ptr(rgba), self.rows, k, C.byref(cnt), C.byref(first)))
        assert cnt.value == k
        return (db, rgba, int(first.value)) if want_rgba else (db, int(first.value))

    def flush(self, want_rgba=False):
        db = np.empty(self.rows, np.float32)
        rgba = np.empty((self.rows, 4), np.uint8) if want_rgba else None
        c = C.c_int64(-2)
        self._chk(self._lib.emspec_column_flush(self._h, _np_ptr(db), _np_ptr(rgba), self.rows, C.byref(c)))
        return (db, rgba, int(c.value)) if want_rgba else (db, int(c.value))

    def reset(self):
        self._chk(self._lib.emspec_reset(self._h))

    # -- live multi-stream streaming: S streams per call, one launch ------------------
    @property
    def live_streams(self):
        return int(self._lib.emspec_live_streams(self._h))

    def _live_out(self, S, cols, want_db, want_rgba, db, rgba):
        shape = (S, self.rows) if cols is None else (S, cols, self.rows)
        if db is None and want_db:
            db = np.empty(shape, np.float32)
        if rgba is None and want_rgba:
            rgba = np.empty(shape + (4,), np.uint8)
        assert db is None or (db.dtype == np.float32 and db.flags.c_contiguous and db.shape == shape)
        assert rgba is None or (rgba.dtype == np.uint8 and rgba.flags.c_contiguous and rgba.shape == shape + (4,))
        return db, rgba

    def columns(self, frames, hop, reassign=True, want_db=True, want_rgba=False, db=None, rgba=None):
        """Per-frame form (emspec_columns): frames [S][n], one frame of every stream -> (db [S][rows] or None,
        rgba [S][rows][4] or None, columns int64 [S] (-1 = the empty column)).  db / rgba: optional preallocated
        (page-locked: PinnedArray.array) outputs."""
        frames = frames if isinstance(frames, np.ndarray) and frames.dtype == np.float32 and frames.flags.c_contiguous \
            else np.ascontiguousarray(frames, np.float32)
        S, n = frames.shape
        db, rgba = self._live_out(S, None, want_db, want_rgba, db, rgba)
        cols = np.empty(S, np.int64)
        self._chk(self._lib.emspec_columns(self._h, _np_ptr(frames), S, n, hop, int(bool(reassign)), _np_ptr(db), _np_ptr(rgba),
                                           self.rows, _np_ptr(cols)))
        return db, rgba, cols

    def columns_flush(self, want_db=True, want_rgba=False, db=None, rgba=None):
        S = self.live_streams
        db, rgba = self._live_out(S, None, want_db, want_rgba, db, rgba)
        cols = np.empty(S, np.int64)
        self._chk(self._lib.emspec_columns_flush(self._h, _np_ptr(db), _np_ptr(rgba), self.rows, _np_ptr(cols)))
        return db, rgba, cols

    def push_columns_multi(self, count, n, hop, reassign=True):
        return int(self._lib.emspec_push_columns_multi(self._h, count, n, hop, int(bool(reassign))))

    def push_samples_multi(self, samples, n, hop, reassign=True, want_db=True, want_rgba=False, db=None, rgba=None,
                           count=None, offset=0):
        """Per-sample-block form (emspec_push_samples_multi): samples [S][>= offset + count] (a window [offset, offset + count)
        of every row is fed) -> (db [S][k][rows], rgba, counts int64 [S], first_columns int64 [S]); k = the largest per-stream
        count (or the second dimension of the preallocated db / rgba)."""
        samples = samples if isinstance(samples, np.ndarray) and samples.dtype == np.float32 and samples.flags.c_contiguous \
            else np.ascontiguousarray(samples, np.float32)
        S, width = samples.shape
        if count is None:
            count = width - offset
        assert 0 <= offset and offset + count <= width
        k = self.push_columns_multi(count, n, hop, reassign)
        if k < 0:
            raise EmspecError(ERR_INVALID_ARG, "invalid fft size / hop")
        if db is not None:
            k = db.shape[1]
        elif rgba is not None:
            k = rgba.shape[1]
        db, rgba = self._live_out(S, k, want_db, want_rgba, db, rgba)
        counts, firsts = np.empty(S, np.int64), np.empty(S, np.int64)
        base = C.c_void_p(samples.ctypes.data + 4 * offset)
        self._chk(self._lib.emspec_push_samples_multi(self._h, base, S, count, width, n, hop, int(bool(reassign)), _np_ptr(db),
                                                      _np_ptr(rgba), self.rows, k, _np_ptr(counts), _np_ptr(firsts)))
        return db, rgba, counts, firsts

    # -- the live session's multi-resolution form: n_low below split_row, n_high above, one column per hop ------------
    def columns_multires(self, frames, n_high, hop, split_row, reassign=True, want_db=True, want_rgba=False, db=None, rgba=None):
        """Per-frame form (emspec_columns_multires): frames [S][n_low] -> (db [S][rows] or None, rgba or None, columns
        int64 [S] (-1 = the empty column)); as `columns`."""
        frames = frames if isinstance(frames, np.ndarray) and frames.dtype == np.float32 and frames.flags.c_contiguous \
            else np.ascontiguousarray(frames, np.float32)
        S, n_low = frames.shape
        db, rgba = self._live_out(S, None, want_db, want_rgba, db, rgba)
        cols = np.empty(S, np.int64)
        self._chk(self._lib.emspec_columns_multires(self._h, _np_ptr(frames), S, n_low, n_high, hop, split_row, int(bool(reassign)),
                                                    _np_ptr(db), _np_ptr(rgba), self.rows, _np_ptr(cols)))
        return db, rgba, cols

    def push_columns_multires(self, count, n_low, n_high, hop, reassign=True):
        return int(self._lib.emspec_push_columns_multires(self._h, count, n_low, n_high, hop, int(bool(reassign))))

    def push_samples_multires(self, samples, n_low, n_high, hop, split_row, reassign=True, want_db=True, want_rgba=False,
                              db=None, rgba=None, count=None, offset=0, max_columns=None):
        """Per-sample-block form (emspec_push_samples_multires): as `push_samples_multi`; max_columns overrides the output
        capacity handed to the library (default: what the block completes, or the preallocated outputs' second dimension)."""
        samples = samples if isinstance(samples, np.ndarray) and samples.dtype == np.float32 and samples.flags.c_contiguous \
            else np.ascontiguousarray(samples, np.float32)
        S, width = samples.shape
        if count is None:
            count = width - offset
        assert 0 <= offset and offset + count <= width
        k = self.push_columns_multires(count, n_low, n_high, hop, reassign)
        if k < 0:   # (the call itself names the rule the shape breaks)
            k = 0
        if db is not None:
            k = db.shape[1]
        elif rgba is not None:
            k = rgba.shape[1]
        db, rgba = self._live_out(S, k, want_db, want_rgba, db, rgba)
        counts, firsts = np.empty(S, np.int64), np.empty(S, np.int64)
        base = C.c_void_p(samples.ctypes.data + 4 * offset)
        self._chk(self._lib.emspec_push_samples_multires(self._h, base, S, count, width, n_low, n_high, hop, split_row,
                                                         int(bool(reassign)), _np_ptr(db), _np_ptr(rgba), self.rows,
                                                         k if max_columns is None else max_columns, _np_ptr(counts),
                                                         _np_ptr(firsts)))
        return db, rgba, counts, firsts

    # -- the live session's multi-band form: 2..4 fft sizes n[0] > ... > n[K-1], band k above split_rows[k-1], one column per hop -
    def _bands(self, n, split_rows=()):
        """(K, the sizes and the split rows as ctypes int32 arrays), kept per ladder: a live call per hop does not rebuild them."""
        key = (tuple(n), tuple(split_rows))
        cache = self.__dict__.setdefault("_band_arrays", {})
        hit = cache.get(key)
        if hit is None:
            if len(cache) >= 64:
                cache.clear()
            hit = cache[key] = (len(key[0]), _i32(key[0]), _i32(key[1]))
        return hit

    def columns_multiband(self, frames, n, split_rows, hop, reassign=True, want_db=True, want_rgba=False, db=None, rgba=None):
        """Per-frame form (emspec_columns_multiband): frames [S][n[0]] -> (db [S][rows] or None, rgba or None, columns
        int64 [S] (-1 = the empty column)); as `columns`."""
        frames = frames if isinstance(frames, np.ndarray) and frames.dtype == np.float32 and frames.flags.c_contiguous \
            else np.ascontiguousarray(frames, np.float32)
        K, sizes, splits = self._bands(n, split_rows)
        S = frames.shape[0]
        db, rgba = self._live_out(S, None, want_db, want_rgba, db, rgba)
        cols = np.empty(S, np.int64)
        self._chk(self._lib.emspec_columns_multiband(self._h, _np_ptr(frames), S, K, sizes, splits, hop,
                                                     int(bool(reassign)), _np_ptr(db), _np_ptr(rgba), self.rows, _np_ptr(cols)))
        return db, rgba, cols

    def push_columns_multiband(self, count, n, hop, reassign=True):
        K, sizes, _ = self._bands(n)
        return int(self._lib.emspec_push_columns_multiband(self._h, count, K, sizes, hop, int(bool(reassign))))

    def push_samples_multiband(self, samples, n, split_rows, hop, reassign=True, want_db=True, want_rgba=False, db=None, rgba=None,
                               count=None, offset=0, max_columns=None):
        """Per-sample-block form (emspec_push_samples_multiband): as `push_samples_multires`."""
        samples = samples if isinstance(samples, np.ndarray) and samples.dtype == np.float32 and samples.flags.c_contiguous \
            else np.ascontiguousarray(samples, np.float32)
        K, sizes, splits = self._bands(n, split_rows)
        S, width = samples.shape
        if count is None:
            count = width - offset
        assert 0 <= offset and offset + count <= width
        k = self.push_columns_multiband(count, n, hop, reassign)
        if k < 0:   # (the call itself names the rule the shape breaks)
            k = 0
        if db is not None:
            k = db.shape[1]
        elif rgba is not None:
            k = rgba.shape[1]
        db, rgba = self._live_out(S, k, want_db, want_rgba, db, rgba)
        counts, firsts = np.empty(S, np.int64), np.empty(S, np.int64)
        base = C.c_void_p(samples.ctypes.data + 4 * offset)
        self._chk(self._lib.emspec_push_samples_multiband(self._h, base, S, count, width, K, sizes, splits, hop,
                                                          int(bool(reassign)), _np_ptr(db), _np_ptr(rgba), self.rows,
                                                          k if max_columns is None else max_columns, _np_ptr(counts),
                                                          _np_ptr(firsts)))
        return db, rgba, counts, firsts

    def reset_stream(self, stream):
        self._chk(self._lib.emspec_reset_stream(self._h, stream))

    # -- overlays of every streaming call above (include/emspec.h: emspec_set_live_peaks / emspec_set_live_wave) ------------
    @staticmethod
    def _overlay_array(out, dtype):
        """out: a PinnedArray or a C-contiguous writable numpy array of float32 or of 8-byte records -> (array, pairs)."""
        arr = out.array if isinstance(out, PinnedArray) else out
        assert isinstance(arr, np.ndarray) and arr.flags.c_contiguous and arr.flags.writeable
        assert arr.dtype == np.float32 or arr.dtype == dtype, arr.dtype
        return arr, arr.nbytes // 8

    def set_live_peaks(self, k, min_db, out):
        """emspec_set_live_peaks: while set, every streaming call also writes the k loudest peaks at or above min_db of each
        column it delivers to out[(s * cols + slot) * k + i] (cols: 1 for the per-frame calls and flushes, the call's max_columns
        for the push calls).  out: a float32 array of (pos, db) pairs, an array of dtype PEAK_DTYPE, or a PinnedArray of either
        (written in place by the kernel); None clears.  The engine keeps a reference while it is set."""
        if out is None:
            self._chk(self._lib.emspec_set_live_peaks(self._h, 0, 0.0, None, 0))
            self._live_peaks = None
            return
        arr, pairs = self._overlay_array(out, PEAK_DTYPE)
        self._chk(self._lib.emspec_set_live_peaks(self._h, int(k), float(min_db), _np_ptr(arr), pairs))
        self._live_peaks = out

    def set_live_wave(self, out):
        """emspec_set_live_wave: while set, every streaming call also writes the (lo, hi) envelope pair of the samples under each
        column it delivers to out[s * cols + slot].  out as for set_live_peaks (dtype WAVE_DTYPE); None clears.  Set it before
        the sessions' first frames (or after reset())."""
        if out is None:
            self._chk(self._lib.emspec_set_live_wave(self._h, None, 0))
            self._live_wave = None
            return
        arr, pairs = self._overlay_array(out, WAVE_DTYPE)
        self._chk(self._lib.emspec_set_live_wave(self._h, _np_ptr(arr), pairs))
        self._live_wave = out

    @staticmethod
    def _record_array(out, dtype):
        """out: a PinnedArray or a C-contiguous writable numpy array of `dtype` records (or of bytes) -> (array, records)."""
        arr = out.array if isinstance(out, PinnedArray) else out
        assert isinstance(arr, np.ndarray) and arr.flags.c_contiguous and arr.flags.writeable
        assert arr.dtype == dtype or arr.dtype == np.uint8, arr.dtype
        return arr, arr.nbytes // dtype.itemsize

    def set_live_level(self, out):
        """emspec_set_live_level: while set, every streaming call also writes the level record (LEVEL_DTYPE: exact sum of squares
        in two limbs, peak, odd count) of the samples under each column it delivers to out[s * cols + slot].  out: an array of
        LEVEL_DTYPE (or of bytes), 8-byte aligned, or a PinnedArray of either (written in place by the kernel); None clears.
        Set it before the sessions' first frames (or after reset()).  level_values() / level_sum() turn records into dB."""
        if out is None:
            self._chk(self._lib.emspec_set_live_level(self._h, None, 0))
            self._live_level = None
            return
        arr, records = self._record_array(out, LEVEL_DTYPE)
        self._chk(self._lib.emspec_set_live_level(self._h, _np_ptr(arr), records))
        self._live_level = out

    def set_live_cross(self, views, a, b, out):
        """emspec_set_live_cross: while set, every streaming call also writes the cross record (CROSS_DTYPE) of the streams
        p views + a and p views + b under each column it delivers to out[p * cols + slot].  out as for set_live_level; None
        clears.  While it is set, reset_stream() is refused (ERR_STATE): the streams of a pair restart together."""
        if out is None:
            self._chk(self._lib.emspec_set_live_cross(self._h, 0, 0, 0, None, 0))
            self._live_cross = None
            return
        arr, records = self._record_array(out, CROSS_DTYPE)
        self._chk(self._lib.emspec_set_live_cross(self._h, int(views), int(a), int(b), _np_ptr(arr), records))
        self._live_cross = out

    # -- live history (include/emspec.h: emspec_set_live_history / emspec_history_view) ----------------------------------------
    def set_live_history(self, columns):
        """emspec_set_live_history: keep the last `columns` delivered dB columns of every stream of both sessions on the device
        (0 clears).  Set it before the sessions' first frames (or after reset())."""
        self._chk(self._lib.emspec_set_live_history(self._h, int(columns)))

    def live_history(self, stream=0, session="multi"):
        """emspec_live_history: (end, first) - the columns the stream has emitted and the first one its ring holds - or None
        without a history, for a session that has not started or a stream it does not have."""
        first = C.c_int64(-1)
        end = int(self._lib.emspec_live_history(self._h, _SESSIONS[session], int(stream), C.byref(first)))
        return None if end < 0 else (end, int(first.value))

    @staticmethod
    def _view_map(map):
        """None, a ViewMap, a (db_top, db_range, gate_db, shift_db) tuple or a dict of those names -> ViewMap or None."""
        if map is None or isinstance(map, ViewMap):
            return map
        if isinstance(map, dict):
            return ViewMap(float(map["db_top"]), float(map["db_range"]), float(map["gate_db"]), float(map.get("shift_db", 0.0)))
        return ViewMap(*(float(x) for x in map))

    def history_view_device(self, first_column, factor, groups, stream0=0, streams=None, map=None, db=None, index=None, rgba=None,
                            session="multi", stream=None):
        """emspec_history_view_device: db [streams][groups][rows] float32 / index uint8 / rgba [..][4] uint8 contiguous CUDA
        tensors or None (not all).  Enqueues on `stream` (a torch.cuda.Stream; default: the current torch stream); does not
        synchronise."""
        import torch
        sess = _SESSIONS[session]
        if streams is None:
            streams = (self.live_streams if sess == SESSION_MULTI else 1) - stream0
        for t in (db, index, rgba):
            assert t is None or (t.is_cuda and t.is_contiguous())
        st = stream if stream is not None else torch.cuda.current_stream()
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        m = self._view_map(map)
        self._chk(self._lib.emspec_history_view_device(self._h, sess, int(stream0), int(streams), int(first_column), int(factor),
                                                       int(groups), C.byref(m) if m is not None else None, ptr(db), ptr(index),
                                                       ptr(rgba), C.c_void_p(st.cuda_stream)))

    def history_view(self, first_column, factor, groups, stream0=0, streams=None, map=None, want=("db",), db=None, index=None,
                     rgba=None, session="multi"):
        """emspec_history_view: groups of `factor` stored columns from first_column on, of streams [stream0, stream0 + streams)
        (default: all from stream0 on) -> {"db": [streams][groups][rows] float32, "index": uint8, "rgba": [..][4] uint8}, each
        present when named in `want` or preallocated (numpy arrays or PinnedArray.array, written in place)."""
        sess = _SESSIONS[session]
        if streams is None:
            streams = (self.live_streams if sess == SESSION_MULTI else 1) - stream0
        shape = (max(int(streams), 0), max(int(groups), 0), self.rows)
        if db is None and "db" in want:
            db = np.empty(shape, np.float32)
        if index is None and "index" in want:
            index = np.empty(shape, np.uint8)
        if rgba is None and "rgba" in want:
            rgba = np.empty(shape + (4,), np.uint8)
        for a, dt, sh in ((db, np.float32, shape), (index, np.uint8, shape), (rgba, np.uint8, shape + (4,))):
            assert a is None or (a.dtype == dt and a.flags.c_contiguous and a.shape == sh), (a.dtype, a.shape, sh)
        m = self._view_map(map)
        self._chk(self._lib.emspec_history_view(self._h, sess, int(stream0), int(streams), int(first_column), int(factor),
                                                int(groups), C.byref(m) if m is not None else None, _np_ptr(db), _np_ptr(index),
                                                _np_ptr(rgba)))
        return {"db": db, "index": index, "rgba": rgba}

    # -- stereo image (include/emspec.h: emspec_stereo_*) -----------------------------------------------------
    STEREO_OUTPUTS = ("level", "index", "pan", "rgba")

    def stereo_default_map(self):
        """emspec_stereo_default_map: the engine's configuration, shift 0, pan_range_db = 12, as a StereoMap."""
        m = StereoMap()
        self._chk(self._lib.emspec_stereo_default_map(self._h, C.byref(m)))
        return m

    def set_stereo_colormap(self, palette):
        """emspec_set_stereo_colormap: uint8 [33][256][4] (make_stereo_colormap builds the engine's own law)."""
        palette = np.ascontiguousarray(palette, np.uint8)
        assert palette.shape == (STEREO_PAN_LEVELS, 256, 4)
        self._chk(self._lib.emspec_set_stereo_colormap(self._h, _np_ptr(palette)))

    @staticmethod
    def _stereo_tensors(shape, device, want, given):
        """The four outputs as CUDA tensors: those given, those named in `want` allocated, the others None."""
        import torch
        out = {}
        for name in Engine.STEREO_OUTPUTS:
            t = given.get(name)
            if t is None and name in want:
                t = torch.empty(shape + ((4,) if name == "rgba" else ()), dtype=torch.float32 if name == "level" else torch.uint8,
                                device=device)
            assert t is None or (t.is_cuda and t.is_contiguous())
            out[name] = t
        return out

    @staticmethod
    def _stereo_arrays(shape, want, given):
        """The four outputs as numpy arrays: those given (numpy arrays or PinnedArray.array, written in place), those named in
        `want` allocated, the others None."""
        out = {}
        for name in Engine.STEREO_OUTPUTS:
            a = given.get(name)
            sh, dt = shape + ((4,) if name == "rgba" else ()), np.float32 if name == "level" else np.uint8
            if a is None and name in want:
                a = np.empty(sh, dt)
            assert a is None or (a.dtype == dt and a.flags.c_contiguous and a.shape == sh), (name, a.dtype, a.shape, sh)
            out[name] = a
        return out

    def stereo_device(self, db_t, views=2, a=0, b=1, map=None, want=("index", "pan"), stream=None, **given):
        """emspec_stereo_device: db_t a contiguous float32 CUDA tensor [pairs * views, ...] -> {"level", "index", "pan", "rgba"}
        CUDA tensors [pairs, ...] (rgba + [4]): those named in `want` or passed as keywords.  Enqueues; does not synchronise."""
        import torch
        assert db_t.is_cuda and db_t.dtype == torch.float32 and db_t.is_contiguous() and db_t.dim() >= 1
        streams = db_t.shape[0]
        cells = db_t.numel() // streams if streams else 0
        assert views > 0 and streams % views == 0
        out = self._stereo_tensors((streams // views,) + tuple(db_t.shape[1:]), db_t.device, want, given)
        st = stream if stream is not None else torch.cuda.current_stream(db_t.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        m = _stereo_map(map)
        self._chk(self._lib.emspec_stereo_device(self._h, ptr(db_t), streams // views, int(views), int(a), int(b), cells,
                                                 C.byref(m) if m is not None else None, ptr(out["level"]), ptr(out["index"]),
                                                 ptr(out["pan"]), ptr(out["rgba"]), C.c_void_p(st.cuda_stream)))
        return out

    def batch_stereo_device(self, pcm_t, n, hop, reassign=True, views=2, a=0, b=1, map=None, want=("index", "pan"), stream=None,
                            **given):
        """emspec_batch_stereo_device: pcm_t a contiguous float32 CUDA tensor [S, L], S % views == 0 -> the stereo image of the
        dB batch_device would deliver, CUDA tensors [S / views, columns, rows].  Enqueues; does not synchronise."""
        import torch
        assert pcm_t.is_cuda and pcm_t.dtype == torch.float32 and pcm_t.is_contiguous() and pcm_t.dim() == 2
        S, L = pcm_t.shape
        out = self._stereo_tensors((S // max(int(views), 1), num_columns(L, n, hop), self.rows), pcm_t.device, want, given)
        st = stream if stream is not None else torch.cuda.current_stream(pcm_t.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        m = _stereo_map(map)
        self._chk(self._lib.emspec_batch_stereo_device(self._h, ptr(pcm_t), S, L, n, hop, int(bool(reassign)), int(views), int(a),
                                                       int(b), C.byref(m) if m is not None else None, ptr(out["level"]),
                                                       ptr(out["index"]), ptr(out["pan"]), ptr(out["rgba"]), C.c_void_p(st.cuda_stream)))
        return out

    def batch_pcm_stereo(self, src, fmt, n, hop, reassign=True, a=0, b=1, map=None, want=("index", "pan"), **given):
        """emspec_batch_pcm_stereo: raw frames as batch_pcm takes them -> the stereo image of each source's views a and b, numpy
        arrays [sources, columns, rows] (rgba + [4]); only the requested outputs cross PCIe on the way out."""
        src, sources, frames = _pcm_rows(src, fmt)
        out = self._stereo_arrays((sources, max(num_columns(frames, n, hop), 0), self.rows), want, given)
        m = _stereo_map(map)
        self._chk(self._lib.emspec_batch_pcm_stereo(self._h, _np_ptr(src), C.byref(fmt), sources, frames, n, hop, int(bool(reassign)),
                                                    int(a), int(b), C.byref(m) if m is not None else None, _np_ptr(out["level"]),
                                                    _np_ptr(out["index"]), _np_ptr(out["pan"]), _np_ptr(out["rgba"])))
        return out

    def _stereo_pairs(self, sess, stream0, pairs, views):
        return ((self.live_streams if sess == SESSION_MULTI else 1) - stream0) // max(int(views), 1) if pairs is None else int(pairs)

    def history_view_stereo_device(self, first_column, factor, groups, views=2, a=0, b=1, stream0=0, pairs=None, map=None,
                                   want=("index", "pan"), session="multi", stream=None, **given):
        """emspec_history_view_stereo_device: the stereo image of the history's groups, CUDA tensors [pairs][groups][rows].
        Enqueues on `stream` (default: the current torch stream); does not synchronise."""
        import torch
        sess = _SESSIONS[session]
        pairs = self._stereo_pairs(sess, stream0, pairs, views)
        out = self._stereo_tensors((max(pairs, 0), max(int(groups), 0), self.rows), "cuda", want, given)
        st = stream if stream is not None else torch.cuda.current_stream()
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        m = _stereo_map(map)
        self._chk(self._lib.emspec_history_view_stereo_device(self._h, sess, int(stream0), pairs, int(views), int(a), int(b),
                                                              int(first_column), int(factor), int(groups),
                                                              C.byref(m) if m is not None else None, ptr(out["level"]), ptr(out["index"]),
                                                              ptr(out["pan"]), ptr(out["rgba"]), C.c_void_p(st.cuda_stream)))
        return out

    def history_view_stereo(self, first_column, factor, groups, views=2, a=0, b=1, stream0=0, pairs=None, map=None,
                            want=("index", "pan"), session="multi", **given):
        """emspec_history_view_stereo: for each pair (streams stream0 + p views + a / + b) the peak hold of each channel's groups
        of `factor` stored columns, then the stereo law -> numpy arrays [pairs][groups][rows] (rgba + [4])."""
        sess = _SESSIONS[session]
        pairs = self._stereo_pairs(sess, stream0, pairs, views)
        out = self._stereo_arrays((max(pairs, 0), max(int(groups), 0), self.rows), want, given)
        m = _stereo_map(map)
        self._chk(self._lib.emspec_history_view_stereo(self._h, sess, int(stream0), pairs, int(views), int(a), int(b),
                                                       int(first_column), int(factor), int(groups),
                                                       C.byref(m) if m is not None else None, _np_ptr(out["level"]),
                                                       _np_ptr(out["index"]), _np_ptr(out["pan"]), _np_ptr(out["rgba"])))
        return out

    # -- live audio history (include/emspec.h: emspec_set_live_audio / emspec_audio_view / emspec_audio_batch) ------------------
    def _audio_streams(self, sess, stream0, streams):
        return (self.live_streams if sess == SESSION_MULTI else 1) - stream0 if streams is None else int(streams)

    def set_live_audio(self, samples):
        """emspec_set_live_audio: keep the last `samples` samples every streaming call was fed, per stream of both sessions, on
        the device (0 clears).  Set it before the sessions' first samples (or after reset())."""
        self._chk(self._lib.emspec_set_live_audio(self._h, int(samples)))

    def live_audio(self, stream=0, session="multi"):
        """emspec_live_audio: (end, first) - the samples of the stream that were stored and the first one its ring holds - or
        None without an audio history, for a session that has not started or a stream it does not have."""
        first = C.c_int64(-1)
        end = int(self._lib.emspec_live_audio(self._h, _SESSIONS[session], int(stream), C.byref(first)))
        return None if end < 0 else (end, int(first.value))

    def audio_view_device(self, first_sample, count, pcm, stream0=0, streams=None, stride=None, session="multi", stream=None):
        """emspec_audio_view_device: samples [first_sample, first_sample + count) of streams [stream0, stream0 + streams) into
        the float32 CUDA tensor `pcm` (any 4-byte alignment - a slice will do), rows `stride` samples apart (default: count).
        Enqueues on `stream` (a torch.cuda.Stream; default: the current torch stream); does not synchronise."""
        import torch
        sess = _SESSIONS[session]
        assert pcm is None or (pcm.is_cuda and pcm.dtype == torch.float32)
        st = stream if stream is not None else torch.cuda.current_stream()
        self._chk(self._lib.emspec_audio_view_device(self._h, sess, int(stream0), self._audio_streams(sess, stream0, streams),
                                                     int(first_sample), int(count), C.c_void_p(pcm.data_ptr()) if pcm is not None else None,
                                                     int(count if stride is None else stride), C.c_void_p(st.cuda_stream)))

    def audio_view(self, first_sample, count, stream0=0, streams=None, pcm=None, stride=None, session="multi"):
        """emspec_audio_view: samples [first_sample, first_sample + count) of streams [stream0, stream0 + streams) (default: all
        from stream0 on) -> float32 [streams][stride] (default stride: count; a numpy array or PinnedArray.array given as `pcm`
        is written in place), bit for bit what the session was fed."""
        sess = _SESSIONS[session]
        streams = self._audio_streams(sess, stream0, streams)
        stride = int(count if stride is None else stride)
        if pcm is None:
            pcm = np.zeros((max(streams, 0), max(stride, 0)), np.float32)
        assert pcm.dtype == np.float32 and pcm.flags.c_contiguous
        self._chk(self._lib.emspec_audio_view(self._h, sess, int(stream0), streams, int(first_sample), int(count), _np_ptr(pcm), stride))
        return pcm

    def audio_batch_device(self, first_sample, count, n, hop, reassign=True, stream0=0, streams=None, db=None, rgba=None, index=None,
                           session="multi", stream=None):
        """emspec_audio_batch_device: batch_device over the held samples [first_sample, first_sample + count) of the streams -
        at any n, hop and reassign, not only the session's.  db / rgba / index: contiguous CUDA tensors [streams][columns][rows]
        (+[4]) or None, as for batch_device.  Enqueues on `stream` (default: the current torch stream); does not synchronise."""
        import torch
        sess = _SESSIONS[session]
        for t in (db, rgba, index):
            assert t is None or (t.is_cuda and t.is_contiguous())
        st = stream if stream is not None else torch.cuda.current_stream()
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._chk(self._lib.emspec_audio_batch_device(self._h, sess, int(stream0), self._audio_streams(sess, stream0, streams),
                                                      int(first_sample), int(count), int(n), int(hop), 1 if reassign else 0, ptr(db),
                                                      ptr(rgba), ptr(index), C.c_void_p(st.cuda_stream)))

    def audio_batch(self, first_sample, count, n, hop, reassign=True, stream0=0, streams=None, want=("db",), session="multi"):
        """emspec_audio_batch: the same with host outputs -> {"db": [streams][columns][rows] float32, "rgba": [..][4] uint8,
        "index": uint8}, each present when named in `want`; columns = num_columns(count, n, hop), reduced by the engine's time
        reduction."""
        sess = _SESSIONS[session]
        streams = self._audio_streams(sess, stream0, streams)
        cols = max(num_columns(int(count), int(n), int(hop)), 0)
        f = int(self._lib.emspec_time_reduce(self._h))
        cols = (cols + f - 1) // f if f > 1 else cols
        shape = (max(streams, 0), cols, self.rows)
        db = np.empty(shape, np.float32) if "db" in want else None
        rgba = np.empty(shape + (4,), np.uint8) if "rgba" in want else None
        index = np.empty(shape, np.uint8) if "index" in want else None
        out = Out(_np_ptr(db), _np_ptr(rgba), _np_ptr(index))
        self._chk(self._lib.emspec_audio_batch(self._h, sess, int(stream0), streams, int(first_sample), int(count), int(n), int(hop),
                                               1 if reassign else 0, C.byref(out)))
        return {"db": db, "rgba": rgba, "index": index}
