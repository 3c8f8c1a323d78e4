"""Case table of the small_to_large census (test_s2l_census_cpu.py, test_gpu_s2l_census.py): the windows, the oracle's
answers with their traces, and a restatement in Python integers and floats of what picks the code path of an event in
k_small_to_large_pair and k_small_to_large (pyperiod_amd/csrc/ph_s2l.h, ph_device.h, ph_pair.h, period_hip.hip).
`classify` turns a case and its oracle trace into the set of CLASSES labels it reaches; the CPU census asserts that the
table as a whole reaches every label, so the GPU test can say which event paths it ran.

A case is a dict: name, n, thresh, n_periods (None: N // 2), dtype, trunc, orth, misaligned (the batch starts one double
into its storage), kinds (one word per window) and `claims`, the labels its entry in the table is there for.  Its
windows are seeded by its name alone (persistent: by the window index), so the census and the GPU test build the same
arrays.  Window kinds:
  noise            Gaussian noise
  plant:a,b,..     zero-mean random patterns tiled at the periods a, b, .. (amplitude after '*', default 1) + 0.05 noise
  collapse:p0      2^36 x an integer pattern of period p0 (a power of two) + integer noise in [-3, 3] + integer patterns
                   of periods 24 and 100; the second half of the big pattern is minus the first, so that no shorter
                   period sees it: every column sum and every mean of the first accepted period is exact in
                   fp64 in ANY order of summation, so the residual after the collapse is the same bits in the kernel
                   and in the oracle
  stagnate:p:d     +-(1 + d 2^-23) with one random sign per residue mod p, 32 < p < 64: exactly p-periodic, and the float
                   screen loses d 2^-23 of every sample once a lane's running sum has passed 2 d (see float_screen_small)
  zeros, const     all 0.0, all 0.75
  nan, inf         the planted window of the case with x[17] = NaN / +Inf
  2^k              the planted window of the case times 2^k (k = 400, -400, 510: the sum of squares overflows)
"""

import math
import zlib
from fractions import Fraction

import numpy as np

from oracle import period_oracle as po
from short_windows_cases import CAP32, CAP64, MARGIN32, MARGIN64  # noqa: F401  (the project's margin rule)

SEED = 20262
TOL, TOL32 = 1e-10, 1e-4  # the suite's bars for float64 and float32 windows
CUS = 256  # compute units of an MI355X: the persistent case of the CPU census (the GPU test reads the device's)
DEFAULT_CAP = 16  # PeriodEngine.small_to_large's default capacity

# ------------------------------------------------------------------------------------------------------------------
# Restatements.  Constants: ph_device.h:27 kBlockWide, :267-268 kSplitMax / kSplitMinRows, :403 kPad, :28 kMaxWaves;
# ph_s2l.h:47 kFlatBatch, :119 kS2LBatch; ph_pair.h:864 kPairStaleMeanSq.
# ------------------------------------------------------------------------------------------------------------------
K_BLOCK_WIDE, K_SPLIT_MAX, K_SPLIT_MIN_ROWS, K_PAD, K_MAX_WAVES = 512, 64, 32, 256, 16
K_FLAT_BATCH, K_S2L_BATCH, K_STALE_MEAN_SQ = 8, 32, 9.0e-13
LDS_LIMIT = 160 * 1024  # period_hip.hip:1136
WIDTHS = (512, 256)


def split_G(N, p, width):
    """ph_device.h:271-277 (split_row_means): threads a residue's rows are dealt to."""
    rows = (N + p - 1) // p
    G = 1
    if rows >= K_SPLIT_MIN_ROWS:
        while 2 * G * p <= width and G < K_SPLIT_MAX and rows >= 2 * G * (K_SPLIT_MIN_ROWS // 2):
            G <<= 1
    return G


def split_label(N, p, width):
    """ph_device.h:276-277: which condition ended the doubling at G = 1."""
    G = split_G(N, p, width)
    if G > 1:
        return f"w{width}: G = {G}"
    return f"w{width}: G = 1, rows < 32" if (N + p - 1) // p < K_SPLIT_MIN_ROWS else f"w{width}: G = 1, 2p > width"


def combine_trips(G):
    """ph_device.h:294: trips of `for (k0 = 0; k0 < G; k0 += 16)`."""
    return (G + 15) // 16 if G > 1 else 0


def means_store(p, pair):
    """ph_s2l.h:495-498 (pair kernel: msm up to kEx / 2, prt up to kEx, the column loop beyond) and ph_s2l.h:207-209
    (one-window kernel: msm up to kBlockWide at any block size)."""
    if p > K_BLOCK_WIDE:
        return "column loop"
    return "prt" if pair and p > K_BLOCK_WIDE // 2 else "msm"


def flat_trips(N, width):
    """ph_s2l.h:59 / :87: trips of `for (n0 = tid; n0 < N; n0 += kFlatBatch * width)` for thread 0, and whether
    some thread below `width` has none (N < width)."""
    return -(-N // (K_FLAT_BATCH * width)), N < width


def copy_path(N, base_offset_bytes):
    """ph_s2l.h:296 (s2l_copy); the LDS buffer and the rows of the HBM workspace (win_stride: multiples of 4 doubles) are
    16-byte aligned, so the source row x + w N decides: 'vector' or 'scalar'."""
    return "vector" if base_offset_bytes % 16 == 0 and N % 2 == 0 else "scalar"


def copy_whole_trips(N, block):
    """ph_s2l.h:299-300: whether nv = N / 2 is a multiple of the 4 blockDim vectors of one trip."""
    return (N // 2) % (4 * block) == 0


def usable(rsq):
    """ph_pair.h:852."""
    return 0.0 < rsq < 1.79e308


def pick_scale(rsq, N):
    """ph_pair.h:855-860."""
    if not usable(rsq):
        return 1.0
    e = math.frexp(rsq / N)[1]
    return math.ldexp(1.0, -(e >> 1))


def stale(rsq, sc, N):
    """ph_pair.h:865-867, ph_s2l.h:538."""
    return usable(rsq) and rsq * sc * sc < K_STALE_MEAN_SQ * N


def threshold_A(rn, dn, thresh, N):
    """ph_s2l.h:345 (set_thresholds): the branch is `A > 0.0`."""
    return (rn - (thresh - 1e-13) * dn) * math.sqrt(N)


def float_screen_small(x, p):
    """ph_pair.h:620-655 (pair_partial_small) for 32 < p < 64, where G = 64 / p = 1, in numpy float32 on the float image
    of ph_s2l.h:382-383: lane j adds rows 0, 2, .. and 1, 3, .. of its residue in two chains (four rows per trip, the
    rest into the first), then the two, then the ragged tail; z = sum_j tot_j^2 w_j -- the last sum here in float64,
    the kernel's tree of six float adds is within 4e-7 of it.  -> z at the scale of the image, the scale."""
    f = np.float32
    n = len(x)
    assert 32 < p < 64
    sc = pick_scale(float(np.sum(x * x)), n)
    img = (x * sc).astype(f)
    full, rows = n // p, -(-n // p)
    nfull = p - (rows * p - n)
    z = 0.0
    for j in range(p):
        s0, s1, r = f(0), f(0), 0
        while r + 4 <= full:
            s0 = f(s0 + img[r * p + j])
            s1 = f(s1 + img[(r + 1) * p + j])
            s0 = f(s0 + img[(r + 2) * p + j])
            s1 = f(s1 + img[(r + 3) * p + j])
            r += 4
        while r < full:
            s0 = f(s0 + img[r * p + j])
            r += 1
        tot = f(f(s0 + s1) + (img[full * p + j] if full * p + j < n else f(0)))
        w = f(1.0 / rows) if j < nfull else f(1.0 / (rows - 1))
        z += float(f(f(tot * tot) * w))
    return z, sc


def flag_bound_without_kappa(rsq, rn, dn, thresh, n, sc):
    """ph_s2l.h:344-358 with every kappa zero: the bound T0 - 2^-20 |T0| the screen value is compared with (A > 0)."""
    A = threshold_A(rn, dn, thresh, n)
    assert A > 0
    T0 = (rsq - A * A * (1.0 + 1e-12)) * sc * sc
    return T0 - 9.5367431640625e-07 * abs(T0)


def carve(n, elem):
    """ph_device.h:1081."""
    return (n * elem + 15) & ~15


def pair_lds_bytes(N):
    """ph_s2l.h:283-286."""
    return (carve(N + K_PAD, 8) + carve(N, 8) + carve(2 * K_MAX_WAVES, 8) + carve(K_BLOCK_WIDE // 2, 8) + carve(K_BLOCK_WIDE, 8) +
            carve(8, 8) + carve(4, 4) + carve(4, 4) + carve(8, 4))


ENGINES = {  # name -> environment of ph_create (period_hip.hip:1148-1171)
    "pair": {},
    "pair512": {"PH_S2L_BLOCK": 512},
    "one": {"PH_S2L_PAIR": 0},
    "one256": {"PH_S2L_PAIR": 0, "PH_SWEEP_BLOCK": 256},
    "hbm": {"PH_HBM_WINDOW": 1},
}
PAIR_ENGINES, ONE_ENGINES = ("pair", "pair512"), ("one", "one256", "hbm")


def plan_variant(dtype, general, N, n_periods, env=()):
    """period_hip.hip:694-712 (plan_small_to_large) with :589-602: -> (variant, block, window) as 'pair' / 'one', threads,
    'lds' / 'hbm'.  `env` is an ENGINES entry."""
    env = dict(env)
    s2l_pair, hbm = int(env.get("PH_S2L_PAIR", 1)) != 0, int(env.get("PH_HBM_WINDOW", 0)) != 0
    sweep_block, s2l_block = int(env.get("PH_SWEEP_BLOCK", K_BLOCK_WIDE)), int(env.get("PH_S2L_BLOCK", 1024))
    sz = np.dtype(dtype).itemsize
    lds = (carve(N + K_PAD, sz) + (carve(N, sz) if general else carve(K_BLOCK_WIDE, sz)) + carve(2 * K_MAX_WAVES, 8) +
           carve(K_S2L_BATCH, 8) + carve(4, 4))
    if general and (hbm or lds > LDS_LIMIT):
        lds -= (N * sz + 15) & ~15
    window = "lds" if not hbm and lds <= LDS_LIMIT else "hbm"
    pair = (s2l_pair and np.dtype(dtype) == np.float64 and not general and window == "lds" and 2 <= n_periods < N and
            sweep_block >= 512 and pair_lds_bytes(N) <= LDS_LIMIT)
    return ("pair", s2l_block, window) if pair else ("one", sweep_block, window)


def resident_pairs(N, block, cus):
    """period_hip.hip:1645-1646: workgroups of the persistent pair kernel."""
    return cus * max(1, min(LDS_LIMIT // pair_lds_bytes(N), 2048 // block))


# ------------------------------------------------------------------------------------------------------------------
# Windows
# ------------------------------------------------------------------------------------------------------------------
def _rng(name, w):
    return np.random.default_rng([SEED, zlib.crc32(name.encode()), w])


def _plant(rng, n, spec, noise=0.05):
    t = np.arange(n)
    x = noise * rng.standard_normal(n)
    for item in spec.split(","):
        p, _, amp = item.partition("*")
        pat = rng.standard_normal(int(p))
        x += float(amp or 1.0) * (pat - pat.mean())[t % int(p)]
    return x


COLLAPSE_BIG = 2.0 ** 36


def collapse_parts(name, w, n, p0):
    """The integer parts of a collapse window: (big pattern of period p0 before the 2^36, everything else)."""
    rng = _rng(name, w)
    t = np.arange(n)
    half = rng.integers(1, 9, p0 // 2) * rng.choice([-1, 1], p0 // 2)
    big = np.concatenate([half, -half])  # no component at a shorter period: p0 is the first period that takes it
    small = rng.integers(-3, 4, n) + rng.integers(-6, 7, 24)[t % 24] + rng.integers(-6, 7, 100)[t % 100]
    return big[t % p0].astype(np.int64), small.astype(np.int64)


def _window(case, w, kind, planted):
    n, name = case["n"], case["name"]
    rng = _rng(name, w)
    if kind == "noise":
        return rng.standard_normal(n)
    if kind.startswith("plant:"):
        return _plant(rng, n, kind[6:])
    if kind.startswith("collapse:"):
        big, small = collapse_parts(name, w, n, int(kind[9:]))
        return COLLAPSE_BIG * big.astype(np.float64) + small.astype(np.float64)
    if kind.startswith("stagnate:"):
        p, d = (int(v) for v in kind[9:].split(":"))
        return (rng.choice([-1.0, 1.0], p) * (1.0 + d * 2.0 ** -23))[np.arange(n) % p]
    if kind == "zeros":
        return np.zeros(n)
    if kind == "const":
        return np.full(n, 0.75)
    base = _plant(rng, n, planted)
    if kind in ("nan", "inf"):
        base[17] = np.nan if kind == "nan" else np.inf
        return base
    if kind.startswith("2^"):
        return base * 2.0 ** int(kind[2:])
    raise AssertionError(kind)


_WIN = {}


def persistent_windows(W, n=48):
    """Window w: noise + a pattern of period 2 + w % 23, seeded by w."""
    key = ("persistent", W)
    if key not in _WIN:
        x = np.empty((W, n))
        for w in range(W):
            x[w] = _plant(np.random.default_rng([SEED, 48, w]), n, str(2 + w % 23), noise=1.0 if w % 5 == 4 else 0.3)
        x.setflags(write=False)
        _WIN[key] = x
    return _WIN[key]


def windows(case, W=None):
    """(W, N) windows of the case in its dtype (float32: the float64 windows rounded).  `W`: the persistent case only."""
    if case["kinds"] == "persistent":
        return persistent_windows(W or 8 * CUS + 3, case["n"])
    if case["name"] not in _WIN:
        x = np.stack([_window(case, w, k, case.get("planted", "3,7,40,100")) for w, k in enumerate(case["kinds"])])
        x = x.astype(case["dtype"])
        x.setflags(write=False)
        _WIN[case["name"]] = x
    return _WIN[case["name"]]


# ------------------------------------------------------------------------------------------------------------------
# The table
# ------------------------------------------------------------------------------------------------------------------
def _case(name, n, thresh, kinds, n_periods=None, dtype=np.float64, trunc=False, orth=False, misaligned=False, claims=(),
          **extra):
    return dict(name=name, n=n, thresh=thresh, n_periods=n_periods, kinds=tuple(kinds) if kinds != "persistent" else kinds,
                dtype=dtype, trunc=trunc, orth=orth, misaligned=misaligned, claims=tuple(claims), **extra)


P4096 = "plant:3,7,12,40,100,130,300,500,700"
PA, PB = "plant:3,16,128,512", "plant:7,49,343"  # accepts of PA divide 3 x 2^k, those of PB are multiples of 7
STRONG = "plant:5*2,64"
DEGENERATE = ("zeros", "const", "nan", "inf", "2^400", "2^-400", "2^510")
N_EDGE = 60


def _table():
    t = []
    g = lambda w, *gs: [f"w{w}: G = {k}" for k in gs]
    # accept-all: every period of both windows is an event, and every epoch swaps the staging buffer with a dirty write-back
    t.append(_case("accept_all_0", 1100, 0.0, ("noise", "noise"), 1099, claims=g(512, 2, 4, 8, 16, 32) + [
        "thresh == 0", "count > cap", "pair: both accept the same p", "w512: G = 1, rows < 32", "accepted p == 64",
        "accepted p == 256", "accepted p == 257", "accepted p == 512", "accepted p == 513", "accepted p > 513", "accepted p | N",
        "accepted p > N / 2 (two rows)", "accepted p == N - 1", "means: msm", "means: prt", "means: column loop",
        "n_periods == N - 1 (pair kernel)"]))
    t.append(_case("accept_all_neg", 1100, -1.0, ("noise", "noise"), 1099, claims=["thresh < 0", "count > cap"]))
    t.append(_case("accept_4100", 4100, 0.0, ("noise", "noise"), 40, claims=g(512, 16, 32, 64) + g(256, 4, 8, 16, 32, 64) + [
        "w512: flat trips 2 (N = 4100)", "combine loop: 2+ trips"]))
    t.append(_case("accept_4097", 4097, 0.0, ("noise", "noise"), 24, claims=["w512: flat trips 2 (N = 4097)", "copy: scalar, N odd"]))
    t.append(_case("accept_2049", 2049, 0.0, ("noise", "noise"), 24, claims=["w256: flat trips 2 (N = 2049)", "copy: scalar, N odd"]))
    t.append(_case("accept_300", 300, 0.0, ("noise", "noise", "noise"), 299, claims=["flat: partial trip (N < width)", "w256: G = 2",
                                                                                   "lone last window accepts 2+"]))
    # planted
    t.append(_case("planted_same", 4096, 0.05, (P4096, P4096), 800, claims=g(512, 64, 32, 16, 4, 2) + [
        "pair: both accept the same p", "A > 0 throughout", "accepted p < 64", "accepted p > 64", "w256: G = 1, 2p > width",
        "copy: 16-byte vectors", "copy: nv no multiple of 4 blockDim", "flat: one trip"]))
    t.append(_case("planted_disjoint", 4096, 0.05, (PA, PB), 800, claims=["pair: interleaved disjoint accepts"]))
    t.append(_case("planted_misaligned", 4096, 0.05, (PA, PB, P4096), 800, misaligned=True, claims=["copy: scalar, base at 8 mod 16"]))
    t.append(_case("planted_lone", 1000, 0.05, (PA, PB, "plant:3,7,40,100"), claims=["lone last window accepts 2+"]))
    t.append(_case("only_window_0", 4096, 0.3, (STRONG, "noise"), 600, claims=["pair: only window 0 accepts"]))
    t.append(_case("only_window_1", 4096, 0.3, ("noise", STRONG), 600, claims=["pair: only window 1 accepts"]))
    t.append(_case("neither", 4096, 0.3, ("noise", "noise"), 600, claims=["pair: neither accepts"]))
    t.append(_case("long_257", 7968, 0.05, ("plant:257", "plant:5,257"), 260, claims=["w512: G = 1, 2p > width"]))
    # the float screen of period 33 is 3e-6 short of the fp64 value, more than the 2^-20 the thresholds give away on their
    # own: the accept is found only because the flag test widens its bound by kappa_q
    t.append(_case("kappa_33", 7968, 0.9995, ("stagnate:33:31", "plant:5,257"), 40, claims=["flag only through kappa_q", "pair: only window 0 accepts"]))
    t.append(_case("thresh_1", 1000, 1.0, (PA, PB), claims=["thresh >= 1"]))
    t.append(_case("thresh_1.5", 1000, 1.5, (PA, PB), claims=["thresh >= 1", "A <= 0 with periods left"]))
    # collapse: thresh 0.05 (nothing after it), a threshold between the noise and the planted 24 / 100, and -1
    for p0 in ((2, 8), (4, 16)):
        t.append(_case(f"collapse_hi_{p0[0]}_{p0[1]}", 4096, 0.05, (f"collapse:{p0[0]}", f"collapse:{p0[1]}"), 120,
                       claims=["rescale after an accept", "A <= 0 with periods left"]))
    # below 0.05 a period before p0 > 2 may be accepted, and its means are not exact: p0 = 2 only.  The neighbour is a noise
    # window, which accepts every period at these thresholds.
    t.append(_case("collapse_mid_a", 4096, COLLAPSE_MID["collapse_mid_a"], ("collapse:2", "noise"), 120, claims=["rescale after an accept"]))
    t.append(_case("collapse_mid_b", 4096, COLLAPSE_MID["collapse_mid_b"], ("noise", "collapse:2"), 120, claims=["rescale after an accept"]))
    t.append(_case("collapse_neg_2_2", 4096, -1.0, ("collapse:2", "collapse:2"), 120, claims=["rescale after an accept", "thresh < 0"]))
    # degenerate windows as the second and as the first member of a pair
    label = {"zeros": "window of zeros", "const": "residual exactly zero after an accept", "nan": "NaN sample", "inf": "+Inf sample",
             "2^400": "scale 2^400", "2^-400": "scale 2^-400", "2^510": "sum of squares overflows"}
    for k in DEGENERATE:
        t.append(_case(f"degenerate_{k}_second", 1000, 0.05, ("plant:3,7,40,100", k), claims=[label[k]]))
        t.append(_case(f"degenerate_{k}_first", 1000, 0.05, (k, "plant:3,7,40,100"), claims=[label[k]]))
    # ticket edges: n_periods around the 16 wavefronts of the first tickets, and the switch to the one-window kernel
    for npd in (2, 3, 15, 16, 17, 18, N_EDGE - 1, N_EDGE, N_EDGE + 3):
        name = {N_EDGE - 1: "N - 1 (pair kernel)", N_EDGE: "N (one-window kernel)", N_EDGE + 3: "N + 3 (one-window kernel)"}.get(npd, str(npd))
        t.append(_case(f"n_periods_{npd}", N_EDGE, 0.02, ("plant:2,3,16", "plant:3,5,17", "plant:2,15,18"), npd, claims=[f"n_periods == {name}"]))
    t.append(_case("persistent", 48, 0.05, "persistent", claims=["more pairs than resident workgroups", "lone last window accepts 2+"]))
    # float32 windows and the trunc / orth modes: the one-window kernel
    t.append(_case("f32_planted_4096", 4096, 0.05, (PA, PB), 800, dtype=np.float32, claims=["float32"]))
    t.append(_case("f32_planted_1100", 1100, 0.05, ("plant:3,7,40,100,300,530*1.5", PB), 600, dtype=np.float32, claims=["float32", "accepted p > 513"]))
    t.append(_case("f32_planted_2049", 2049, 0.05, (PA, PB), dtype=np.float32, claims=["float32", "w256: flat trips 2 (N = 2049)"]))
    t.append(_case("trunc_1000", 1000, 0.05, (PA, PB), trunc=True, claims=["trunc"]))
    t.append(_case("orth_1000", 1000, 0.05, (PA, PB), orth=True, claims=["orth"]))
    t.append(_case("trunc_orth_1100", 1100, 0.05, ("plant:3,7,40,100,300", PB), 400, trunc=True, orth=True, claims=["trunc", "orth"]))
    return t


# Thresholds of the two collapse windows that are screened on after the collapse: chosen by a scan of the oracle so that
# the planted 24 and 100 are accepted and every decision of the window is 20 % and more away from the threshold
# (test_s2l_census_cpu.py holds them to 1e-3).
COLLAPSE_MID = {"collapse_mid_a": 4.3e-12, "collapse_mid_b": 7.6e-13}

CASES = tuple(_table())
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# knife edges: one accepted period of the case per class, thresh = that period's imposed x (1 -+ 1e-12); see knife_cases()
KNIFE_CASE = "planted_same"
KNIFE_CLASSES = ("G >= 16", "prt", "column loop")


def knife_class(n, p):
    return "G >= 16" if p <= K_BLOCK_WIDE and split_G(n, p, 512) >= 16 else means_store(p, True) if p > K_BLOCK_WIDE // 2 else None


CLASSES = tuple(
    [f"w{w}: G = {k}" for w in WIDTHS for k in (2, 4, 8, 16, 32, 64)]
    + [f"w{w}: G = 1, {why}" for w in WIDTHS for why in ("rows < 32", "2p > width")]
    + ["combine loop: 2+ trips"]
    + ["accepted p < 64", "accepted p == 64", "accepted p > 64"]
    + [f"accepted p == {p}" for p in (256, 257, 512, 513)] + ["accepted p > 513"]
    + ["means: msm", "means: prt", "means: column loop"]
    + ["accepted p | N", "accepted p ragged (nfull < p)", "accepted p > N / 2 (two rows)", "accepted p == N - 1"]
    + ["flat: one trip", "flat: partial trip (N < width)", "w512: flat trips 2 (N = 4097)", "w512: flat trips 2 (N = 4100)",
       "w256: flat trips 2 (N = 2049)"]
    + ["copy: 16-byte vectors", "copy: scalar, N odd", "copy: scalar, base at 8 mod 16", "copy: nv no multiple of 4 blockDim"]
    + ["pair: both accept the same p", "pair: only window 0 accepts", "pair: only window 1 accepts", "pair: neither accepts",
       "pair: interleaved disjoint accepts", "lone last window accepts 2+"]
    + ["A > 0 throughout", "A <= 0 with periods left", "rescale after an accept", "residual exactly zero after an accept"]
    + ["thresh == 0", "thresh < 0", "thresh >= 1", "window of zeros", "NaN sample", "+Inf sample", "sum of squares overflows",
       "scale 2^400", "scale 2^-400", "count > cap", "flag only through kappa_q"]
    + [f"n_periods == {k}" for k in (2, 3, 15, 16, 17, 18, "N - 1 (pair kernel)", "N (one-window kernel)", "N + 3 (one-window kernel)")]
    + ["more pairs than resident workgroups", "float32", "trunc", "orth"]
)


# ------------------------------------------------------------------------------------------------------------------
# The oracle's answers
# ------------------------------------------------------------------------------------------------------------------
_REF = {}


def n_periods_of(case):
    return case["n"] // 2 if case["n_periods"] is None else case["n_periods"]


def general(case):
    return bool(case["trunc"] or case["orth"])


def oracle_window(x, case, thresh=None):
    """The oracle on one window (float64 samples): dict of periods, powers, bases, events, margin.  `margin` is the
    smallest |imposed - thresh| / |thresh| over the periods, for thresh == 0 the smallest |imposed| -- the same number
    held absolutely; 1.0 where no period gives a finite value."""
    thresh = case["thresh"] if thresh is None else thresh
    tr = {}
    with np.errstate(all="ignore"):
        per, pw, bs = po.small_to_large(np.asarray(x, dtype=np.float64), thresh, n_periods_of(case), case["trunc"], case["orth"], trace=tr)
    ev = tr["events"]
    margin = tr["min_margin"]
    if thresh == 0:
        margin = min([abs(e[1]) for e in ev if e[1] == e[1]], default=1.0)
    return dict(periods=[int(p) for p in per], powers=np.array(pw, dtype=np.float64), events=ev, margin=float(margin),
                bases=np.array(bs, dtype=np.float64).reshape(len(per), len(x)))


def ref(case, W=None):
    """One oracle_window per window of the case: computed once and shared."""
    key = (case["name"], W)
    if key not in _REF:
        _REF[key] = [oracle_window(row, case) for row in windows(case, W).astype(np.float64)]
    return _REF[key]


def bar(case):
    return MARGIN64 if case["dtype"] == np.float64 else MARGIN32


def admitted(case, W=None):
    """Whether every window of the case takes part in the same-period-list comparison."""
    return all(r["margin"] >= bar(case) for r in ref(case, W))


def accept_scales(r, x):
    """Per accepted period k of an oracle_window: (||r_k|| / ||x||, max|r_k|) of the residual before the accept."""
    by_p = {e[0]: e for e in r["events"]}
    dn = po.periodic_norm(np.asarray(x, dtype=np.float64))
    return [(by_p[p][3] / dn, by_p[p][4]) for p in r["periods"]]


def _knife_threshold(x, case, p, t):
    """A threshold t with imposed(p) == t when the oracle runs at t (1 - 1e-12), or None: a threshold that moves changes
    which earlier periods are accepted and with them the residual, so the period's own value is iterated to a fixed point."""
    for _ in range(6):
        ev = {e[0]: e for e in oracle_window(x, case, t * (1 - 1e-12))["events"]}
        if ev[p][1] == t:
            return t
        t = ev[p][1]
        if not t > 0:
            return None
    return None


_KNIFE = []


def knife_cases():
    """-> [(name, base case, window, period, thresh, accepts)]: for each of KNIFE_CLASSES the first accepted period of
    KNIFE_CASE (windows in order, periods ascending) that has such a threshold, 1e-12 below it (the period is accepted)
    and above (it is not)."""
    if not _KNIFE:
        case = BY_NAME[KNIFE_CASE]
        for cls in KNIFE_CLASSES:
            found = None
            for w, r in enumerate(ref(case)):
                x = windows(case)[w].astype(np.float64)
                for p, pw in zip(r["periods"], r["powers"]):
                    t = _knife_threshold(x, case, p, float(pw)) if knife_class(case["n"], p) == cls else None
                    if t is not None:
                        found = (w, p, t)
                        break
                if found:
                    break
            assert found, ("no knife edge", cls)
            w, p, t = found
            _KNIFE.append((f"{KNIFE_CASE}[{w}] p={p} below", case, w, p, t * (1 - 1e-12), True))
            _KNIFE.append((f"{KNIFE_CASE}[{w}] p={p} above", case, w, p, t * (1 + 1e-12), False))
    return list(_KNIFE)


# ------------------------------------------------------------------------------------------------------------------
# classify
# ------------------------------------------------------------------------------------------------------------------
def _window_labels(case, kind, r, x):
    n, thresh = case["n"], case["thresh"]
    out = set()
    for p in r["periods"]:
        if not general(case):
            for width in WIDTHS:
                if p <= K_BLOCK_WIDE:
                    out.add(split_label(n, p, width))
                    trips, partial = flat_trips(n, width)
                    if trips == 2 and n in (4097, 4100, 2049):
                        out.add(f"w{width}: flat trips 2 (N = {n})")
                    if width == 512:
                        out.add("flat: partial trip (N < width)" if partial else "flat: one trip" if trips == 1 else "flat: 2+ trips")
                    if combine_trips(split_G(n, p, width)) >= 2:
                        out.add("combine loop: 2+ trips")
            if case["dtype"] == np.float64:
                out.add("means: " + means_store(p, True))
        out.add("accepted p < 64" if p < 64 else "accepted p == 64" if p == 64 else "accepted p > 64")
        if p in (256, 257, 512, 513):
            out.add(f"accepted p == {p}")
        if p > 513:
            out.add("accepted p > 513")
        out.add("accepted p | N" if n % p == 0 else "accepted p ragged (nfull < p)")
        if n / 2 < p < n:
            out.add("accepted p > N / 2 (two rows)")
        if p == n - 1:
            out.add("accepted p == N - 1")
    # the state of the flag test along the trace (ph_s2l.h:344-361, :538-543)
    ev = r["events"]
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        rsq0 = float(np.sum(x * x))
    if ev and math.isfinite(rsq0) and rsq0 > 0:
        dn = ev[0][3]
        sc = pick_scale(rsq0, n)
        signs = []
        for i, e in enumerate(ev):
            signs.append(threshold_A(e[3], dn, thresh, n) > 0)
            if e[2] and i + 1 < len(ev):
                tsq = ev[i + 1][3] ** 2 * n
                if stale(tsq, sc, n):
                    out.add("rescale after an accept")
                    sc = pick_scale(tsq, n)
                if tsq == 0.0:
                    out.add("residual exactly zero after an accept")
        out.add("A > 0 throughout" if all(signs) else "A <= 0 with periods left")
    if len(r["periods"]) > DEFAULT_CAP:
        out.add("count > cap")
    if kind.startswith("stagnate:") and r["periods"] and 32 < r["periods"][0] < 64:
        e = {v[0]: v for v in ev}[r["periods"][0]]
        z, sc = float_screen_small(x, e[0])
        if z * (1 + 5e-7) < flag_bound_without_kappa(e[3] ** 2 * n, e[3], ev[0][3], thresh, n, sc) * (1 - 2.0 ** -23):
            out.add("flag only through kappa_q")
    out |= {"zeros": {"window of zeros"}, "nan": {"NaN sample"}, "inf": {"+Inf sample"}, "2^510": {"sum of squares overflows"},
            "2^400": {"scale 2^400"}, "2^-400": {"scale 2^-400"}}.get(kind, set())
    return out


def classify(case, W=None):
    """The labels of CLASSES (and a few more) the case reaches, from its shape and its oracle trace."""
    n, npd, thresh = case["n"], n_periods_of(case), case["thresh"]
    x = windows(case, W)
    rs = ref(case, W)
    kinds = case["kinds"] if case["kinds"] != "persistent" else ("plant",) * len(rs)
    out = set()
    for w, (kind, r) in enumerate(zip(kinds, rs)):
        out |= _window_labels(case, kind, r, x[w])
    plan = plan_variant(case["dtype"], general(case), n, npd)
    if plan[0] == "pair":
        for w in range(len(rs)):
            base = 8 * w * n + (8 if case["misaligned"] else 0)
            path = copy_path(n, base)
            out.add("copy: 16-byte vectors" if path == "vector" else "copy: scalar, N odd" if n % 2 else "copy: scalar, base at 8 mod 16")
            if path == "vector" and not (copy_whole_trips(n, 1024) and copy_whole_trips(n, 512)):
                out.add("copy: nv no multiple of 4 blockDim")
        for a in range(0, len(rs) - 1, 2):
            p0, p1 = rs[a]["periods"], rs[a + 1]["periods"]
            if set(p0) & set(p1):
                out.add("pair: both accept the same p")
            if p0 and not p1:
                out.add("pair: only window 0 accepts")
            if p1 and not p0:
                out.add("pair: only window 1 accepts")
            if not p0 and not p1:
                out.add("pair: neither accepts")
            if len(p0) >= 2 and len(p1) >= 2 and not set(p0) & set(p1) and min(p1) < max(p0) and min(p0) < max(p1):
                out.add("pair: interleaved disjoint accepts")
        if len(rs) % 2 and len(rs[-1]["periods"]) >= 2:
            out.add("lone last window accepts 2+")
        if (len(rs) + 1) // 2 > max(resident_pairs(n, 1024, CUS), resident_pairs(n, 512, CUS)):
            out.add("more pairs than resident workgroups")
    out.add("thresh == 0" if thresh == 0 else "thresh < 0" if thresh < 0 else "thresh >= 1" if thresh >= 1 else "0 < thresh < 1")
    if npd in (2, 3, 15, 16, 17, 18):
        out.add(f"n_periods == {npd}")
    if npd == n - 1 and plan[0] == "pair":
        out.add("n_periods == N - 1 (pair kernel)")
    if npd == n and plan[0] == "one":
        out.add("n_periods == N (one-window kernel)")
    if npd == n + 3 and plan[0] == "one":
        out.add("n_periods == N + 3 (one-window kernel)")
    if case["dtype"] == np.float32:
        out.add("float32")
    if case["trunc"]:
        out.add("trunc")
    if case["orth"]:
        out.add("orth")
    return out


# ------------------------------------------------------------------------------------------------------------------
# The reference's own rounding: the accepted periods replayed in longdouble
# ------------------------------------------------------------------------------------------------------------------
def headroom(case, w, W=None):
    """The oracle's accepted periods of window w evaluated again in longdouble (the same accepts, the same expressions):
    -> the largest |power - power_ld| / (||r_k|| / ||x||) and the largest |base - base_ld| / max|r_k| over the accepts,
    the units of the GPU test's bars."""
    ld = np.longdouble
    r = ref(case, W)[w]
    res = windows(case, W)[w].astype(ld)
    n = ld(res.size)
    norm = lambda v: np.sqrt(np.sum(v * v)) / np.sqrt(n)
    with np.errstate(all="ignore"):
        dn = norm(res)
        worst_p = worst_b = 0.0
        for k, p in enumerate(r["periods"]):
            base = po.project(res, p, case["trunc"], case["orth"])
            trial = res - base
            rn = norm(res)
            imposed = (rn - norm(trial)) / dn
            top = np.max(np.abs(res))
            if rn > 0:
                worst_p = max(worst_p, float(abs(ld(r["powers"][k]) - imposed) / (rn / dn)))
            if top > 0:
                worst_b = max(worst_b, float(np.max(np.abs(r["bases"][k].astype(ld) - base)) / top))
            res = trial
    return worst_p, worst_b


def collapse_exact(case, w):
    """For a collapse window: the first accepted period, and whether the oracle's base of it equals the rational column
    means exactly and its fp64 residual equals the rational residual (Fraction arithmetic)."""
    kind = case["kinds"][w]
    p0 = int(kind[9:])
    big, small = collapse_parts(case["name"], w, case["n"], p0)
    exact = [Fraction(int(COLLAPSE_BIG)) * int(b) + int(s) for b, s in zip(big, small)]
    r = ref(case)[w]
    first = r["periods"][0]
    cols = [exact[j::first] for j in range(first)]
    means = [sum(c, Fraction(0)) / len(c) for c in cols]
    base_ok = all(Fraction(float(v)) == means[i % first] for i, v in enumerate(r["bases"][0]))
    x = windows(case)[w]
    resid_ok = all(Fraction(float(x[i] - r["bases"][0][i])) == exact[i] - means[i % first] for i in range(case["n"]))
    return first, base_ok, resid_ok
