"""The plain reference of the d = 1 map (sympgpr_amd/csrc/map.hip: applymap_kernel), numpy and the CPU oracle only: the two sums
K*(1,:).alpha, K*(2,:).alpha in long double with a bound on what any fp64 evaluation of them may differ by, the one-step
checks that restart from the device's own rows (so chaos never enters a tolerance), a host restatement of map_step's call
sequence, and the problems the team tests run (tests/test_applymap_team_cpu.py asserts their preconditions without a GPU,
tests/test_gpu_applymap_team.py runs them).

Every tolerance here is derived, none is measured on the code under test:
  B = (n0 u + 3e-13) T + 4e-15 max|K*| |alpha|_1,  T = |K*| |alpha|,  u = 2^-53
    n0 u T covers the summation error of ANY order of adding n0 fp64 products; the rest is the project's elementwise Gram
    tolerance (gram_close in tests/test_gpu_device_ops.py: |dK| <= 4e-15 max|K| + 3e-13 |K|) carried through the sum.
  explicit step   |Praw - (p - r1(q, p))| <= B1 + 4 u max(1, |p|)
  implicit step   |r1(q, Praw) - p + Praw| <= 4 tol max(1, |Praw|) + 2 B1,  tol = 1e-13: the secant leaves with
    |P1 - P0| <= tol scale, so |f~(P0)| <= 2 tol scale for a slope <= 1.5 with noisy secant slopes and |f(P1)| <= that
    + 1.5 tol scale + B1; the reference's own evaluation adds another B1.  Precondition (CPU test): |dr1/dP| <= 0.5.
  q update        Q against q + r2(q, p_next), modulo 2 pi under WRAP_Q, within B2 + 4 u max(2 pi, |q| + |r2|)
  WRAP_P          p_next in [0, 2 pi) and (Praw - p_next) / 2 pi within 8 u max(1, |Praw|) of an integer
Praw is recovered from pdiff: Praw = p_i + (pd_{i+1} - pd_i); without WRAP_P it must also be p_next up to the four roundings of
that recovery, 4 u max(1, |p|, |Praw|, |pd_i|, |pd_{i+1}|).

The number of rows calls is comparable between device and reference only where no test of the secant's stopping rule falls
near its threshold.  About one orbit-step in twenty does, so no seed gives hundreds of clear orbits: the start points are
chosen per orbit (clear_starts) and recorded (problem)."""
import functools
import os

import numpy as np

U = 2.0 ** -53
TOL = 1e-13                      # map.hip: the secant's stopping tolerance
TWO_PI = 2.0 * np.pi
WRAP_Q, WRAP_P, EXPLICIT, LOSS_NEGP = 1, 2, 4, 8
C_ALPHA = 0.3                    # alpha = (c / sqrt(n0)) N(0, 1): a map near the identity whose sums cancel heavily
HYP = {"A": (1.2, 1.5, 1.0), "B": (1.2, 1.5, 1.0), "C": (1.2, 1.5, 1.0), "D": (1.2, 1.5, 0.7, 1.0)}


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle()


# ---- reference sums

def sums(fam, hyp, xt, yt, alpha, q, P, bounds=True):
    """r1 = K*(1,:).alpha, r2 = K*(2,:).alpha at the points (q, P) (vectors), K* from the oracle's build_K, added in long double;
    B1, B2 the bounds of the module docstring.  -> r1, r2, B1, B2 (float64 vectors; B1 = B2 = None without `bounds`)"""
    orc = _oracle()
    q, P = np.atleast_1d(np.asarray(q, dtype=np.float64)), np.atleast_1d(np.asarray(P, dtype=np.float64))
    n, n0 = len(q), len(xt)
    a = np.asarray(alpha, dtype=np.longdouble)
    absa, norm1 = np.abs(a), float(np.abs(a).sum())
    out = np.zeros((4, n))
    for s in range(0, n, 256):
        e = min(n, s + 256)
        m = e - s
        K = orc.build_K(fam, q[s:e], P[s:e], xt, yt, hyp, threads=4)              # (2 m, 2 n0): rows m.. are K*(2,:)
        Kl = K.astype(np.longdouble)
        out[:2, s:e] = (Kl @ a).astype(np.float64).reshape(2, m)
        if bounds:
            T = (np.abs(Kl) @ absa).astype(np.float64).reshape(2, m)
            kmax = np.abs(K).max(axis=1).reshape(2, m).max(axis=0) if n0 else np.zeros(m)
            out[2:, s:e] = (n0 * U + 3e-13) * T + 4e-15 * kmax * norm1
    return (out[0], out[1], out[2], out[3]) if bounds else (out[0], out[1], None, None)


def guess(fam, hypp, xp, yp, alphap, q, p):
    """the regular GP's first guess of P at (q, p): K*reg.alphap, added in long double"""
    q, p = np.atleast_1d(np.asarray(q, dtype=np.float64)), np.atleast_1d(np.asarray(p, dtype=np.float64))
    K = _oracle().buildKreg(fam, q, p, xp, yp, hypp, threads=4)
    return (K.astype(np.longdouble) @ np.asarray(alphap, dtype=np.longdouble)).astype(np.float64)


# ---- problems

def training(fam, n0, n0p, seed):
    """cheap training data that need no factorisation: points uniform in [0, 2 pi) x [-1, 1], random weights"""
    rng = np.random.default_rng(seed)
    d = dict(fam=fam, hyp=np.array(HYP[fam]), hypp=np.array(HYP[fam]) * np.array([1.05, 0.95] + [1.0] * (len(HYP[fam]) - 2)),
             xt=rng.uniform(0, TWO_PI, n0), yt=rng.uniform(-1, 1, n0), alpha=C_ALPHA / np.sqrt(n0) * rng.standard_normal(2 * n0),
             xp=rng.uniform(0, TWO_PI, n0p), yp=rng.uniform(-1, 1, n0p),
             alphap=C_ALPHA / np.sqrt(max(n0p, 1)) * rng.standard_normal(n0p))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def starts(kind, ntest, seed):
    rng = np.random.default_rng(seed)
    Q0 = rng.uniform(0.5, 5.5, ntest)
    if kind == "wrapp":                      # a third of the starts at negative momentum: P mod 2 pi really wraps
        P0 = rng.uniform(0.3, 0.7, ntest)
        P0[1::3] = -P0[1::3]
    elif kind == "lossy":                    # close to P = 0: LOSS_NEGP bites, at different steps
        P0 = rng.uniform(0.01, 0.7, ntest)
    else:
        P0 = rng.uniform(-0.5, 0.5, ntest)
    return Q0, P0


class Case:
    def __init__(self, id, ntest, n0, n0p, S, fam="A", mode=WRAP_Q, nm=4, kind="plain", seed=1, want_pdiff=True):
        self.id, self.ntest, self.n0, self.n0p, self.S = id, ntest, n0, n0p, S
        self.fam, self.mode, self.nm, self.kind, self.seed, self.want_pdiff = fam, mode, nm, kind, seed, want_pdiff

    def __repr__(self):
        return self.id


# team geometry: family A, WRAP_Q.  S is for 256 CUs (512 workgroup slots); the GPU test asserts it from the library
GEOMETRY = [
    Case("s1-memory", 520, 1300, 1300, 1),       # 6 rounds from memory, with a value reference
    Case("s2-ragged", 200, 513, 513, 2),         # member 0's second round holds one point
    Case("s2-mixed", 200, 2561, 2561, 2),        # member 0 from memory (6 rounds), member 1 staged (5)
    Case("s2-memory", 200, 2817, 2817, 2),       # both members from memory
    Case("s3", 100, 700, 700, 3),                # last member ragged (188 points)
    Case("s13-config05", 37, 4096, 4096, 13),    # the tokamak geometry at a quarter of its points, 481 of 512 slots
    Case("s16-one", 16, 3841, 3841, 16),         # largest team, last member owns one point
    Case("s16-memory", 16, 20481, 64, 16),       # member 0 from memory; 15 members without guess points
    Case("guess-short", 20, 1500, 300, 6),       # members 2 .. 5 have nrp == 0
    Case("guess-one", 20, 1500, 1, 6),           # one guess point
    Case("guess-long", 20, 300, 3000, 2),        # the guess alone ends staging (nrp = 6)
]
# families and modes, all at the s3 shape
MODES = [
    Case("B-wrapq", 100, 700, 700, 3, fam="B"),                                  # the implicit equation is linear in P
    Case("C-wrapq", 100, 700, 700, 3, fam="C"),
    Case("D-wrapq", 100, 700, 700, 3, fam="D"),
    Case("A-wrapq-wrapp", 100, 700, 700, 3, mode=WRAP_Q | WRAP_P, kind="wrapp"),
    Case("A-wrapq-lossnegp", 100, 700, 700, 3, mode=WRAP_Q | LOSS_NEGP, kind="lossy"),
    Case("B-explicit-wrapp", 100, 700, 0, 3, fam="B", mode=EXPLICIT | WRAP_P, kind="wrapp"),
    Case("C-explicit", 100, 700, 0, 3, fam="C", mode=EXPLICIT),
    Case("A-henon", 100, 700, 700, 3, mode=0),
    Case("A-wrapq-nopdiff", 100, 700, 700, 3, want_pdiff=False),
]
CASES = GEOMETRY + MODES
# the base problems of the zero-weight padding tests: 300 real points, 16 orbits, nm = 2 (S = 2 as they stand)
PADDING = [Case("pad-explicit", 16, 300, 0, 2, mode=EXPLICIT, nm=2), Case("pad-guess", 16, 300, 300, 2, nm=2)]


STARTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_team_starts.npz")


@functools.lru_cache(maxsize=None)
def problem(case_id):
    """the training data and start points of a case, and `calls`, the reference's rows-call count of every step and orbit.
    The start points are recorded (tests/golden/map_team_starts.npz, written by `python tests/ref_map.py`): choosing them
    means iterating the reference over twice as many candidates, seconds that no GPU case should spend;
    tests/test_applymap_team_cpu.py holds the record to the reference."""
    c = next(c for c in CASES + PADDING if c.id == case_id)
    d = training(c.fam, c.n0, c.n0p, 100 + c.seed)
    with np.load(STARTS) as g:
        d["Q0"], d["P0"], d["calls"] = g[c.id + "/Q0"], g[c.id + "/P0"], g[c.id + "/calls"]
    assert d["Q0"].shape == d["P0"].shape == (c.ntest,) and d["calls"].shape == (c.nm - 1, c.ntest)
    return d


def record_starts():
    out = {}
    for c in CASES + PADDING:
        d = training(c.fam, c.n0, c.n0p, 100 + c.seed)
        out[c.id + "/Q0"], out[c.id + "/P0"], out[c.id + "/calls"] = clear_starts(d, c.mode, c.nm, c.kind, c.ntest, 200 + c.seed)
    np.savez(STARTS, **out)


def clear_starts(d, mode, nm, kind, ntest, seed):
    """ntest start points on whose reference trajectory no test of the secant's stopping rule falls within a factor 4 of the
    threshold (is_clear): the first ntest such of 2 ntest + 8 drawn from `seed`.  About one orbit-step in twenty lies
    that close -- the secant's last step lengths spread over decades -- so a batch of hundreds cannot be had from a seed
    alone; the rule is applied per orbit.  The device's iterates differ from the reference's by rounding (1e-16 against a
    threshold of 1e-13), so on these orbits both take the same branches and make the same number of rows calls."""
    Qc, Pc = starts(kind, 2 * ntest + 8, seed)
    o = iterate(d, mode, nm, Qc, Pc, slopes=False)
    keep = np.flatnonzero(is_clear(o))[:ntest]
    assert len(keep) == ntest, "too few clear orbits among the candidates: change the seed"
    return Qc[keep], Pc[keep], o["calls"][:, keep]


def is_clear(o):
    """per orbit: every stopping test of every secant of a trajectory (iterate) a factor 4 away from its threshold"""
    return (np.isnan(o["end"]) | (o["end"] < 0.25)).all(axis=0) & (np.isnan(o["cont"]) | (o["cont"] > 4.0)).all(axis=0)


def _r(d, q, P, bounds=False):
    return sums(d["fam"], d["hyp"], d["xt"], d["yt"], d["alpha"], q, P, bounds=bounds)


# ---- map_step's call sequence on the host

def secant_calls(d, mode, q, p, maxiter=60, tol=TOL):
    """map_step (map.hip) restated for vectors of orbits with the reference sums and the reference guess: the same guess, the
    same two starting residuals, the same secant and stopping rule, the same last call for q.  -> calls (rows calls of the
    step, per orbit), end (|P1 - P0| / (tol scale) at the test that ended the secant), cont (the smallest such ratio at a test
    that went on), Praw (NaN where the orbit is lost), r2 at (q, p_next), root (Praw before LOSS_NEGP looks at its sign)."""
    n = len(q)
    calls, end, cont = np.zeros(n, dtype=int), np.full(n, np.nan), np.full(n, np.inf)
    if mode & EXPLICIT:
        Praw, calls = p - _r(d, q, p)[0], calls + 1
    else:
        P0 = guess(d["fam"], d["hypp"], d["xp"], d["yp"], d["alphap"], q, p)
        f0 = _r(d, q, P0)[0] - p + P0
        P1 = P0 - f0
        f1 = _r(d, q, P1)[0] - p + P1
        calls, act = calls + 2, np.ones(n, dtype=bool)
        for _ in range(maxiter):
            ratio = np.abs(P1 - P0) / (tol * np.maximum(1.0, np.abs(P1)))
            stop = act & ~(ratio > 1.0)
            end[stop], act = ratio[stop], act & ~stop & (f1 - f0 != 0.0)
            if not act.any():
                break
            cont[act] = np.minimum(cont[act], ratio[act])
            Pn = P1[act] - f1[act] * (P1[act] - P0[act]) / (f1[act] - f0[act])
            P0[act], f0[act], P1[act] = P1[act], f1[act], Pn
            f1[act] = _r(d, q[act], P1[act])[0] - p[act] + P1[act]
            calls[act] += 1
        Praw = np.where(np.abs(f1) <= 1e-8 * np.maximum(1.0, np.abs(p)), P1, np.nan)
    root = Praw
    if mode & LOSS_NEGP:
        Praw = np.where(Praw < 0.0, np.nan, Praw)
    pn = Praw - TWO_PI * np.floor(Praw / TWO_PI) if mode & WRAP_P else Praw
    ok = ~np.isnan(Praw)
    calls[ok & (bool(mode & EXPLICIT) | (pn != Praw))] += 1
    r2 = np.full(n, np.nan)
    if ok.any():
        r2[ok] = _r(d, q[ok], pn[ok])[1]
    return calls, end, cont, Praw, r2, root


def iterate(d, mode, nm, Q0, P0, slopes=True):
    """the reference's own trajectory -> dict of [nm] or [nm - 1] rows: q, p, Praw, root, calls, end, cont, slope (the larger
    |dr1/dP|, by a central difference, of (q, p) and (q, Praw))"""
    n = len(Q0)
    out = {k: np.full((nm - 1, n), np.nan) for k in ("Praw", "root", "calls", "end", "cont", "slope")}
    q, p = np.full((nm, n), np.nan), np.full((nm, n), np.nan)
    q[0], p[0] = Q0, P0
    h = 1e-5
    for i in range(nm - 1):
        ok = ~np.isnan(p[i]) & ~np.isnan(q[i])
        if not ok.any():
            break
        qi, pi = q[i, ok], p[i, ok]
        calls, end, cont, Praw, r2, root = secant_calls(d, mode, qi, pi)
        out["calls"][i, ok], out["end"][i, ok], out["cont"][i, ok], out["Praw"][i, ok], out["root"][i, ok] = calls, end, cont, Praw, root
        if slopes:
            slope = np.abs(_r(d, qi, pi + h)[0] - _r(d, qi, pi - h)[0]) / (2 * h)
            Pv = np.where(np.isnan(Praw), pi, Praw)
            slope = np.maximum(slope, np.abs(_r(d, qi, Pv + h)[0] - _r(d, qi, Pv - h)[0]) / (2 * h))
            out["slope"][i, ok] = slope
        pn = Praw - TWO_PI * np.floor(Praw / TWO_PI) if mode & WRAP_P else Praw
        qn = qi + r2
        if mode & WRAP_Q:
            qn = qn - TWO_PI * np.floor(qn / TWO_PI)
        q[i + 1, ok], p[i + 1, ok] = qn, pn
    out["q"], out["p"] = q, p
    out["calls"] = np.nan_to_num(out["calls"]).astype(int)
    return out


def root_minpack(d, q, p):
    """the reference root of f(P) = r1(q, P) - p + P for ONE orbit: MINPACK hybrd (fsolve, xtol 1e-13) from the regular GP's guess"""
    import scipy.optimize
    g0 = guess(d["fam"], d["hypp"], d["xp"], d["yp"], d["alphap"], [q], [p])[0]
    return scipy.optimize.fsolve(lambda P: _r(d, [q], [P[0]])[0][0] - p + P[0], [g0], xtol=1e-13)[0]


# ---- the one-step checks on the device's rows

def check_steps(d, mode, qmap, pmap, pdiff, nan_starts=()):
    """every one-step check of the module docstring on the rows a device run returned, each step restarted from the device's
    own row; without pdiff (modes without WRAP_P only) Praw is p_next itself.  Asserts; -> {check: worst |error| / bound}."""
    nm, n = qmap.shape
    worst = {}

    def within(name, err, bound):
        if len(err):
            k = int(np.argmax(err / bound))
            worst[name] = max(worst.get(name, 0.0), float(err[k] / bound[k]))
            assert np.all(err <= bound), "%s: |error| %.3e > bound %.3e (orbit-local index %d)" % (name, err[k], bound[k], k)

    lost = np.isnan(pmap)
    assert pdiff is not None or not mode & WRAP_P
    assert np.array_equal(np.isnan(qmap), lost) and (pdiff is None or np.array_equal(np.isnan(pdiff), lost))
    assert np.array_equal(pmap[0], d["P0"], equal_nan=True) and np.array_equal(qmap[0], d["Q0"], equal_nan=True)
    assert pdiff is None or np.array_equal(pdiff[0], pmap[0], equal_nan=True)
    start_lost = np.zeros(n, dtype=bool)
    start_lost[list(nan_starts)] = True
    assert np.array_equal(np.isnan(d["P0"]) | np.isnan(d["Q0"]), start_lost)
    for i in range(nm - 1):
        here = ~lost[i] if i else ~start_lost
        assert lost[i + 1][~here].all(), "a lost orbit came back"
        if mode & LOSS_NEGP:                                   # lost exactly where the reference root is negative
            roots = np.array([root_minpack(d, qmap[i, k], pmap[i, k]) for k in np.flatnonzero(here)])
            assert np.all(np.abs(roots) > 1e-6), "a reference root within 1e-6 of 0: the loss is ambiguous"
            assert np.array_equal(lost[i + 1][here], roots < 0.0), "step %d: orbits lost where the reference keeps them, or kept where it loses them" % i
        else:
            assert not lost[i + 1][here].any(), "step %d: an orbit was lost that the reference keeps" % i
        ok = ~lost[i + 1]
        if not ok.any():
            continue
        q, p, Q, pn = qmap[i, ok], pmap[i, ok], qmap[i + 1, ok], pmap[i + 1, ok]
        Praw = p + (pdiff[i + 1, ok] - pdiff[i, ok]) if pdiff is not None else pn
        if mode & EXPLICIT:
            r1, _, B1, _ = _r(d, q, p, True)
            within("explicit", np.abs(Praw - (p - r1)), B1 + 4 * U * np.maximum(1.0, np.abs(p)))
        else:
            r1, _, B1, _ = _r(d, q, Praw, True)
            within("implicit", np.abs(r1 - p + Praw), 4 * TOL * np.maximum(1.0, np.abs(Praw)) + 2 * B1)
        if mode & WRAP_P:
            assert np.all((pn >= 0.0) & (pn < TWO_PI))
            turns = (Praw - pn) / TWO_PI
            within("wrap_p", np.abs(turns - np.round(turns)), 8 * U * np.maximum(1.0, np.abs(Praw)))
        elif pdiff is not None:
            # p_next IS Praw; what is recovered from pdiff differs from it by the four roundings of the recovery
            mag = np.maximum.reduce([np.ones(len(p)), np.abs(p), np.abs(Praw), np.abs(pdiff[i, ok]), np.abs(pdiff[i + 1, ok])])
            within("pdiff", np.abs(pn - Praw), 4 * U * mag)
        _, r2, _, B2 = _r(d, q, pn, True)
        dq = Q - (q + r2)
        if mode & WRAP_Q:
            assert np.all((Q >= 0.0) & (Q < TWO_PI))
            dq = dq - TWO_PI * np.round(dq / TWO_PI)
        within("q", np.abs(dq), B2 + 4 * U * np.maximum(TWO_PI, np.abs(q) + np.abs(r2)))
    return worst


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record_starts()
