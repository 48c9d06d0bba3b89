"""numpy restatement of the PCM decode (include/emspec.h, PCM front end): raw interleaved little-endian
frames -> float32 streams.  Conversion per sample type, then per view acc = mix[v][0] * x_0, acc = acc + mix[v][c] * x_c for
c = 1 .. channels-1, every product and every sum a float32 operation, channels in ascending order, no fused multiply-add.
Lives under tests/ (like multires_ref.py); the product never imports it."""
import numpy as np

S16, S24, S32, F32 = 1, 2, 3, 4
BYTES = {S16: 2, S24: 3, S32: 4, F32: 4}


def frame_bytes(sample_type, channels):
    return BYTES[sample_type] * channels


def s24_pack(values):
    """int array (-2^23 .. 2^23-1) -> uint8 array, 3 bytes per value, little endian."""
    v = np.asarray(values, np.int64) & 0xFFFFFF
    return np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], axis=-1).astype(np.uint8).reshape(*v.shape[:-1], -1) \
        if v.ndim else np.array([v & 255, (v >> 8) & 255, (v >> 16) & 255], np.uint8)


def convert(raw, sample_type):
    """raw: uint8 array whose last axis is a whole number of samples -> float32 array of the converted samples."""
    raw = np.ascontiguousarray(raw, np.uint8)
    if sample_type == S16:
        return raw.view("<i2").astype(np.float32) * np.float32(2.0 ** -15)
    if sample_type == S24:
        b = raw.reshape(*raw.shape[:-1], -1, 3).astype(np.int32)
        s = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
        s = np.where(s & 0x800000, s - (1 << 24), s)        # sign extension from 3 bytes
        return s.astype(np.float32) * np.float32(2.0 ** -23)
    if sample_type == S32:
        return raw.view("<i4").astype(np.float32) * np.float32(2.0 ** -31)   # int32 -> float32 rounds to nearest even
    if sample_type == F32:
        return raw.view("<f4").copy()
    raise ValueError(sample_type)


def decode(raw, sample_type, channels, mix):
    """raw: uint8 [sources][frames * frame_bytes]; mix: [views][channels] -> float32 [sources * views][frames]."""
    raw = np.ascontiguousarray(raw, np.uint8)
    if raw.ndim == 1:
        raw = raw[None]
    mix = np.asarray(mix, np.float32).reshape(-1, channels)
    x = convert(raw, sample_type).reshape(raw.shape[0], -1, channels)      # [sources][frames][channels]
    out = np.empty((raw.shape[0], mix.shape[0], x.shape[1]), np.float32)
    for v in range(mix.shape[0]):
        acc = (mix[v, 0] * x[:, :, 0]).astype(np.float32)
        for c in range(1, channels):
            prod = (mix[v, c] * x[:, :, c]).astype(np.float32)
            acc = (acc + prod).astype(np.float32)
        out[:, v] = acc
    return out.reshape(raw.shape[0] * mix.shape[0], -1)
