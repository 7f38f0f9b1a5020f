"""Event statistics: the definition of include/clsimhip.h ("Event statistics") restated with Python integers only, independent of
the library -- the term from the weight's bit pattern, the sum as an int, the six words by masking, the double through
fractions.Fraction -- and the record sets the CPU and the GPU tests share."""
import struct
from fractions import Fraction

import numpy as np

from clsim_amd import converter as CV

UNIT = 149                      # sums are integers in units of 2^-149
MASK384 = (1 << 384) - 1
COUNTERS = CV.EVENT_STATISTICS_COUNTERS
KINDS = ("+inf", "-inf", "nan")


def bits_of(weight):
    return struct.unpack("<I", struct.pack("<f", weight))[0]


def term(bits, count=1, generated=False):
    """the exact count x w in units of 2^-149 as an int, or "+inf" / "-inf" / "nan" """
    e, f, negative = (bits >> 23) & 255, bits & 0x7fffff, bits >> 31
    if e == 255:
        if f or (generated and count == 0):
            return "nan"
        return "-inf" if negative else "+inf"
    m = f | (1 << 23) if e else f
    s = max(e, 1) - 1
    value = (count * m) << s
    return -value if negative else value


def words_of(value):
    v = value & MASK384         # two's complement by masking
    return [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)]


def value_of(words):
    v = sum(int(w) << (64 * k) for k, w in enumerate(words))
    return v - (1 << 384) if v >> 383 else v


def double_of(value, special=(0, 0, 0)):
    """the delivered double: one rounding to nearest-even of the exact rational"""
    if special[2] or (special[0] and special[1]):
        return float("nan")
    if special[0]:
        return float("inf")
    if special[1]:
        return float("-inf")
    return float(Fraction(value, 1 << UNIT)) + 0.0 if value else 0.0


def double_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def restate(steps, photons, particles=None, masked=None):
    """(records, counters) as CV.EventStatistics.MakeHost returns them"""
    steps = np.asarray(steps, dtype=CV.STEP_DTYPE)
    photons = np.asarray(photons, dtype=CV.PHOTON_DTYPE)
    if particles is None:
        table, index = [(0, 0)], None
    else:
        table = [(int(p["id"]), int(p["frame"])) for p in particles]
        index = {ident: k for k, (ident, _) in enumerate(table)}
    frames = {frame for _, frame in table}
    mask = set()
    for m in (masked if masked is not None else []):
        if int(m["frame"]) in frames:
            mask.add((int(m["frame"]), int(m["stringID"]), int(m["omID"])))
    acc = [{"gc": 0, "ac": 0, "g": 0, "a": 0, "gs": [0, 0, 0], "as": [0, 0, 0]} for _ in table]
    counters = dict.fromkeys(COUNTERS, 0)

    def add(record, side, t):
        if isinstance(t, str):
            record[side + "s"][KINDS.index(t)] += 1
        else:
            record[side] += t

    wbits = steps["weight"].view(np.uint32)
    for num, w, ident in zip(steps["num"].tolist(), wbits.tolist(), steps["id"].tolist()):
        k = 0 if index is None else index.get(ident)
        if k is None:
            counters["unknown_step_particle"] += 1
            continue
        acc[k]["gc"] += num
        add(acc[k], "g", term(w, num, True))
    wbits = photons["weight"].view(np.uint32)
    for w, ident, s, o in zip(wbits.tolist(), photons["id"].tolist(), photons["stringID"].tolist(), photons["omID"].tolist()):
        k = 0 if index is None else index.get(ident)
        if k is None:
            counters["unknown_particle"] += 1
            continue
        if (table[k][1], s, o) in mask:
            counters["masked"] += 1
            continue
        acc[k]["ac"] += 1
        add(acc[k], "a", term(w))
    out = np.zeros(len(table), dtype=CV.EVENT_STATISTICS_DTYPE)
    for k, ((ident, frame), a) in enumerate(zip(table, acc)):
        out[k] = (ident, frame, a["gc"], a["ac"], words_of(a["g"]), words_of(a["a"]), a["gs"], a["as"])
    return out, counters


def same(got, want):
    assert got[1] == want[1]
    assert got[0].dtype == want[0].dtype and got[0].tobytes() == want[0].tobytes()


# ---- record sets ----
def make_steps(num, weight_bits, ident):
    steps = np.zeros(len(num), dtype=CV.STEP_DTYPE)
    steps["num"] = np.asarray(num, dtype=np.uint32)
    steps["weight"] = np.asarray(weight_bits, dtype=np.uint32).view(np.float32)
    steps["id"] = np.asarray(ident, dtype=np.uint32)
    steps["x"] = np.arange(len(num)) % 7          # (fields the stage does not read)
    steps["sourceType"] = 3
    return steps


def make_photons(weight_bits, ident, string_id=None, om_id=None):
    photons = np.zeros(len(weight_bits), dtype=CV.PHOTON_DTYPE)
    photons["weight"] = np.asarray(weight_bits, dtype=np.uint32).view(np.float32)
    photons["id"] = np.asarray(ident, dtype=np.uint32)
    photons["stringID"] = 1 if string_id is None else np.asarray(string_id, dtype=np.int16)
    photons["omID"] = 1 if om_id is None else np.asarray(om_id, dtype=np.uint16)
    photons["numScatters"] = np.arange(len(weight_bits)) % 5
    photons["wavelength"] = 4e-7
    return photons


def every_exponent_bits():
    """both signs of: +-0, the smallest and the largest subnormal, and for every finite biased exponent 1 ... 254 the fractions 0, all
    ones and a mixed pattern"""
    magnitudes = [0, 1, 0x7fffff]
    for e in range(1, 255):
        magnitudes += [e << 23, (e << 23) | 0x7fffff, (e << 23) | ((e * 0x9e3779) & 0x7fffff)]
    return np.array([m | sign for m in magnitudes for sign in (0, 1 << 31)], dtype=np.uint32)


SPECIAL_BITS = np.array([0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff], dtype=np.uint32)     # +-inf, NaNs of both signs
NUMS = (0, 1, 0xffffffff)


def exponent_case(with_specials=False):
    """steps: every weight of every_exponent_bits() (and the specials) with num_photons 0, 1 and 2^32 - 1; photons: every weight"""
    bits = every_exponent_bits()
    if with_specials:
        bits = np.concatenate([bits, SPECIAL_BITS])
    num = np.repeat(np.array(NUMS, dtype=np.uint32), len(bits))
    w = np.tile(bits, len(NUMS))
    return make_steps(num, w, np.zeros(len(w))), make_photons(bits, np.zeros(len(bits)))


def interleaved_case(seed=5, n_steps=900, n_photons=1300):
    """particles 10, 11, ... 16 (consecutive) or 10, 13, 20, 21, 40 (not), interleaved record by record with identifiers the table
    does not have; three frames; masked modules in two of them, and mask entries that name no frame of the table"""
    rng = np.random.default_rng(seed)
    out = {}
    for name, ids in (("consecutive", np.arange(10, 17)), ("scattered", np.array([10, 13, 20, 21, 40]))):
        p = np.zeros(len(ids), dtype=CV.MCPE_PARTICLE_DTYPE)
        p["id"] = ids
        p["frame"] = np.array([7, 2, 900])[np.arange(len(ids)) % 3]
        p["timeShift"] = 1.5
        pool = np.concatenate([ids, [3, 9, 17, 41, 0xffffffff]])
        w = rng.integers(0, 1 << 32, n_steps, dtype=np.uint64).astype(np.uint32)
        w[(w >> 23) & 255 == 255] ^= 1 << 30                   # finite
        steps = make_steps(rng.integers(0, 1000, n_steps), w, pool[rng.integers(0, len(pool), n_steps)])
        w = rng.integers(0, 1 << 32, n_photons, dtype=np.uint64).astype(np.uint32)
        w[(w >> 23) & 255 == 255] ^= 1 << 30
        photons = make_photons(w, pool[rng.integers(0, len(pool), n_photons)], rng.integers(-2, 3, n_photons), rng.integers(1, 4, n_photons))
        masked = np.zeros(7, dtype=CV.MCPE_MASK_DTYPE)
        masked[:] = [(7, 1, 1), (7, -2, 3), (2, 0, 2), (2, 0, 2), (5, 1, 1), (901, 1, 2), (7, 2, 60)]
        out[name] = (steps, photons, p, masked)
    return out


def dyadic_weights(n=5000, seed=11):
    """multiples of 2^-10 below 2^10, both signs: every binary64 partial sum of n <= 2^30 of them is exact"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-(1 << 20) + 1, 1 << 20, n) / 1024.0).astype(np.float32)


def positive_weights(n=20000, seed=12):
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(-30.0, 30.0, n)).astype(np.float32)
