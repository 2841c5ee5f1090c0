"""numpy restatement of the sample formats of include/fsnp_pcm.h, shared by tests/test_host_pcm.py and tests/test_gpu_pcm.py.

Every expected value of the PCM tests is one of these functions applied to an fp32 result the library already produces, so every
comparison is exact."""
import numpy as np


def crafted():
    """fp32 values the model cannot be made to produce on demand, with what FSNP_SAMPLE_S16 makes of them and whether they clip."""
    lsb = 1.0 / 32768.0
    rows = [
        (0.5 * lsb, 0, 0), (-0.5 * lsb, 0, 0),                   # ties go to the even neighbour
        (1.5 * lsb, 2, 0), (-1.5 * lsb, -2, 0), (2.5 * lsb, 2, 0),
        (32766.5 * lsb, 32766, 0),                               # a tie below full scale: even, not clipped
        (32767.5 * lsb, 32767, 1),                               # rounds to 32768: saturates and counts
        (1.0, 32767, 1), (-1.0, -32768, 0),                      # -1.0 is representable, +1.0 is not
        (-1.0 - 2.0 ** -15, -32768, 1),
        (np.inf, 32767, 1), (-np.inf, -32768, 1), (np.nan, 0, 1),
        (2.0 ** -140, 0, 0),                                          # a denormal
        (0.0, 0, 0), (0.25, 8192, 0),
    ]
    v = np.array([r[0] for r in rows], dtype=np.float32)
    assert all(float(a) == r[0] or np.isnan(r[0]) for a, r in zip(v, rows)), "the crafted values must be exact in fp32"
    return v, np.array([r[1] for r in rows], dtype=np.int16), np.array([r[2] for r in rows], dtype=bool)


def quantise_s16(v):
    """FSNP_SAMPLE_S16 out of fp32 v (any shape) -> (int16 array, number of clipped samples): rint (half to even) of v * 32768 in fp32,
    saturated; NaN -> 0; clipped = saturated or NaN."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.rint(v * np.float32(32768.0))
    nan = np.isnan(q)
    clipped = nan | (q > 32767.0) | (q < -32768.0)
    q = np.where(nan, np.float32(0.0), np.clip(q, -32768.0, 32767.0))
    return q.astype(np.int16), int(clipped.sum())


def peak_s16(v):
    """FSNP_SAMPLE_S16_PEAK of ONE clip's own fp32 samples v [L]: the reference CLI's tail, literally; an all-zero clip gives zeros."""
    v = np.asarray(v, dtype=np.float32)
    assert v.ndim == 1 and v.dtype == np.float32
    if np.max(np.abs(v)) == 0:
        return np.zeros(v.shape, dtype=np.int16)
    return np.int16(0.8 * np.iinfo(np.int16).max * v / np.max(np.abs(v)))


def quantise_rows(v, lengths=None):
    """quantise_s16 per row of v [B, n] -> (int16 [B, n], clipped counts int32 [B]); columns >= lengths[b] are 0 and do not count."""
    v = np.asarray(v, dtype=np.float32)
    out, cnt = np.zeros(v.shape, dtype=np.int16), np.zeros(v.shape[0], dtype=np.int32)
    for b in range(v.shape[0]):
        n = v.shape[1] if lengths is None else int(lengths[b])
        out[b, :n], cnt[b] = quantise_s16(v[b, :n])
    return out, cnt


def peak_rows(v, lengths=None):
    """peak_s16 of each row's own [:lengths[b]] -> int16 [B, n], 0 behind it."""
    v = np.asarray(v, dtype=np.float32)
    out = np.zeros(v.shape, dtype=np.int16)
    for b in range(v.shape[0]):
        n = v.shape[1] if lengths is None else int(lengths[b])
        out[b, :n] = peak_s16(v[b, :n])
    return out
