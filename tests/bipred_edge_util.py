"""Edge tables for BDOF and DMVR: reference samples CONSTRUCTED so that every decision of xProcessDMVR / applyBiOptFlow is taken a known number of times
(tests/test_bipred_edges.py asserts that census on the oracle's trace; tests/test_gpu_bipred_edges.py runs the same tables on the device).

Nothing here is drawn from a generator: textures are integer hashes of the position, so VTM_TEST_SEED_OFFSET cannot move a job out of its class.

DMVR.  All a sub-PU ever reads of a reference picture is its (dx+7) x (dy+7) window (xPrefetch), so a job owns one private tile per list that holds exactly
that window (plus a guard ring) and the job's refOff places the tile where the window is fetched from -- also when clipMv moves the fetch.  The 25 matching
costs compare the bilinear copies bil_l[r][c] = copy( window_l[r + 1][c + 1] ), whole-sample vectors: copy( p ) = p << 2 at 8 bits, p at 10 bits and
( p + 2 ) >> 2 at 12 bits.  Two constructions:
  * aligned( o ): both windows show one strong texture, list 0 displaced by -o and list 1 by +o, so the candidate o compares equal samples and every other
    candidate costs far more than 2 * dx * dy; a delta on the COUNTED (even) rows of list 1 sets the cost of o to a chosen value (in steps of 1, at 8 bits of 4).
  * additive( A, B ): list 1 is flat, list 0 is flat + a[x] + b[y] >= 0, so cost( ox, oy ) = scale * ( dy / 2 * A[ox] + dx * B[oy] ) with A the sliding sums of a
    over dx columns and B those of b over the dy / 2 counted rows (even and odd oy use different rows, so they are independent); scale = 4 at 8 bits.  The
    minimum over a sum of two valleys is taken where both are lowest, a tie needs a repeated minimum on one axis, and the parabola of an axis only sees that
    axis -- unless the centre takes part, whose cost is discounted by a quarter (A[0] = 4n, A[-1] = 3n with B[0] = 0 makes the left neighbour TIE the centre).
BDOF.  A job owns one (w+8) x (h+8) tile per list: the 8-tap reach and the one-sample ring around the block."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as ol

PIC_W, PIC_H, CTU = 256, 192, 128
SHAPES = ((8, 16), (16, 8), (16, 16))
DEPTHS = (8, 10, 12)
GUARD = 2
HEAD = 4096      # untouched samples in front of and behind the tiles


def hash_tex(h, w, salt, levels, step, base):
    """A strongly textured h x w patch: an integer hash of the position, base + step * [0, levels)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    return (base + step * ((x * x * 3 + y * y * 5 + x * y * 7 + x * 11 + y * 13 + salt * 17 + (salt * x) % 5 + (salt * y) % 3) % levels)).astype(np.int16)


def clip_mv(hor, ver, x, y):
    """clipMv (Mv.cpp:56-74) at luma position (x, y) of this module's picture."""
    hmax, hmin = (PIC_W + 8 - x - 1) << 4, (-CTU - 8 - x + 1) << 4
    vmax, vmin = (PIC_H + 8 - y - 1) << 4, (-CTU - 8 - y + 1) << 4
    return min(hmax, max(hmin, hor)), min(vmax, max(vmin, ver))


def cost_scale(bd):
    return 4 if bd == 8 else 1


def sample_mult(bd):
    return 4 if bd == 12 else 1


# ---------------------------------------------------------------------------------------------------------------- DMVR windows
def slide(targets, length):
    """A non-negative sequence whose sliding sums over `length` entries are `targets`."""
    n = len(targets)
    seq = [0] * (length + n - 1)
    for k in range(n - 1):
        d = targets[k + 1] - targets[k]
        if d > 0:
            seq[length + k] = d
        else:
            seq[k] = -d
    inner = targets[0] - sum(seq[:n - 1])
    m = length - (n - 1)
    assert inner >= 0 and m >= 1, (targets, length)
    for i in range(m):
        seq[n - 1 + i] = inner // m + (i < inner % m)
    assert [sum(seq[k:k + length]) for k in range(n)] == list(targets)
    return seq


def additive_windows(w, h, bd, A, B, extra=0):
    """Windows of the additive construction for ONE sub-PU (w, h <= 16): A[ox + 2], B[oy + 2] in sample sums.  extra: a sample sum spread over row 4, columns
    4 .. w - 1 of the bilinear area, which every candidate with an EVEN oy counts and no other: their costs rise by scale * extra, in steps of one."""
    a = slide(A, w)
    b = [0] * (h + 4)
    b[0::2] = slide([B[0], B[2], B[4]], h // 2)
    b[1:h + 2:2] = slide([B[1], B[3]], h // 2)
    return profile_windows(w, h, bd, a, b, extra)


def profile_windows(w, h, bd, a, b, extra=0):
    """list 0 = flat + a[col] + b[row] over the (w+4) x (h+4) bilinear area (replicated into the rest of the window), list 1 = flat."""
    flat = 254 if bd == 12 else 64      # ( flat + 2 ) % 4 == 0 at 12 bits: the search copy of flat + 4 * p is that of flat, + p
    p = np.add.outer(np.array(b, np.int64), np.array(a, np.int64))
    for i in range(extra):
        p[4, 4 + i % (w - 4)] += 1
    p *= sample_mult(bd)
    w0 = np.pad(flat + p, ((1, 2), (1, 2)), mode="edge")
    assert w0.shape == (h + 7, w + 7) and w0.max() < (1 << bd)
    return w0.astype(np.int16), np.full((h + 7, w + 7), flat, np.int16)


def aligned_windows(w, h, bd, o, cost, salt):
    """Windows of the aligned construction (w, h <= 16): candidate o = (ox, oy) costs `cost`, undiscounted."""
    ox, oy = o
    step, base = {8: (2, 64), 10: (8, 64), 12: (32, 256)}[bd]
    big = hash_tex(h + 7 + 4, w + 7 + 4, salt, 61, step, base)
    w0 = big[2 - oy:2 - oy + h + 7, 2 - ox:2 - ox + w + 7].copy()
    w1 = big[2 + oy:2 + oy + h + 7, 2 + ox:2 + ox + w + 7].copy()
    assert cost % cost_scale(bd) == 0
    units, n = cost // cost_scale(bd), (h // 2) * w
    d = np.full(n, units // n, np.int64)
    d[(np.arange(units % n) * 37) % n] += 1      # 37 is odd and n a power of two: distinct places
    assert d.sum() == units
    w1[3 - oy:3 - oy + h:2, 3 - ox:3 - ox + w] += (d.reshape(h // 2, w) * sample_mult(bd)).astype(np.int16)
    return w0, w1


# ---------------------------------------------------------------------------------------------------------------- DMVR job specs
def _spec(w, h, label, win, mv=None, pos=None, **more):
    return dict(w=w, h=h, label=label, win=win, mv=mv, pos=pos, **more)


def threshold_values(w, h, bd):
    """name -> (discounted centre cost, raw SAD that gives it).  10 / 12 bits: exact.  8 bits: costs are multiples of 4 and the discounted centre a multiple of
    3, so the nearest reachable value on each side of the threshold."""
    T, step, out = w * h, cost_scale(bd), {}
    for name, thr in (("T", T), ("2T", 2 * T)):
        raws = range(0, 4 * thr, step)
        below = max(r for r in raws if r - (r >> 2) < thr)
        at = min(r for r in raws if r - (r >> 2) >= thr)
        out[name + "-"], out[name] = (below - (below >> 2), below), (at - (at >> 2), at)
    return out


def winner_values(w, h, bd):
    """Undiscounted cost of an off-centre winner just below / at 2 * dx * dy."""
    T2 = 2 * w * h
    return {"2T-": T2 - cost_scale(bd), "2T": T2}


OFFS8 = ((1, 0), (-1, 0), (0, 1), (0, -1), (2, 0), (-2, 1), (1, 2), (-2, -2))


def threshold_specs(bd):
    specs = []
    for (w, h) in SHAPES:
        tv, wv = threshold_values(w, h, bd), winner_values(w, h, bd)
        for name in ("T-", "T", "2T-", "2T"):
            val, raw = tv[name]
            for i in range(4):
                specs.append(_spec(w, h, ("centre", name, val), aligned_windows(w, h, bd, (0, 0), raw, len(specs))))
        for name in ("2T-", "2T"):
            for o in OFFS8:
                specs.append(_spec(w, h, ("winner", name, wv[name], o), aligned_windows(w, h, bd, o, wv[name], len(specs))))
        # the centre's discounted cost AT dx * dy with a cheaper neighbour: the search must run and move (were it skipped, the vector difference would be 0)
        sc = cost_scale(bd)
        val, raw = tv["T"]
        for axis, side in ((0, 1), (0, -1), (1, 1), (1, -1)):
            unit, other = (sc * h // 2, sc * w) if axis == 0 else (sc * w, sc * h // 2)
            n0 = raw // unit
            X = [0] * 5
            X[2], X[2 + side], X[2 - side], X[2 + 2 * side], X[2 - 2 * side] = n0, n0 // 2, n0 + 2, n0 // 2 + n0, n0 + 4
            yb = -(-raw // other)
            Y = [2 * yb, yb, 0, 1, 1 + yb]
            A, B = (X, Y) if axis == 0 else (Y, X)
            specs.append(_spec(w, h, ("centre_moves", val, axis, side), additive_windows(w, h, bd, A, B, (raw - n0 * unit) // sc)))
    # one 32 x 32 PU: early termination / centre at T / BDOF off just below 2T / at 2T in its four sub-PUs
    tv = threshold_values(16, 16, bd)
    wins = [aligned_windows(16, 16, bd, (0, 0), tv[nm][1], 900 + i) for i, nm in enumerate(("T-", "T", "2T-", "2T"))]
    w0, w1 = (np.zeros((39, 39), np.int16) for _ in range(2))
    for l, dst in enumerate((w0, w1)):      # the four windows overlap by 7 samples: the sub-PU's own 16 x 16 block and the nearer half of the overlap
        for s in range(4):
            sy, sx = 16 * (s // 2), 16 * (s % 2)
            ys, xs = (slice(0, 19) if sy == 0 else slice(3, 23)), (slice(0, 19) if sx == 0 else slice(3, 23))
            dst[sy + ys.start:sy + ys.stop, sx + xs.start:sx + xs.stop] = wins[s][l][ys, xs]
    specs.append(_spec(32, 32, ("quad", tuple(("centre", nm, tv[nm][0]) for nm in ("T-", "T", "2T-", "2T"))), (w0, w1)))
    return specs


def _valley(s, m, left, right, far):
    """Five sums with the minimum m at offset s (+-1), m + left / m + right next to it and + far beyond."""
    v = [None] * 5
    i = s + 2
    v[i], v[i - 1], v[i + 1] = m, m + left, m + right
    for k in range(i - 2, -1, -1):
        v[k] = v[k + 1] + far
    for k in range(i + 2, 5):
        v[k] = v[k - 1] + far
    return v


def tie_specs(bd):
    specs = []
    sc = cost_scale(bd)
    for (w, h) in SHAPES:
        T, cu, cv = w * h, sc * h // 2, sc * w
        # -- off-centre winners at (+-1, +-1): per axis a division result of either sign or the next candidate tying (+8)
        combos = [(a, b) for a in ("div+", "div-", "tie") for b in ("div+", "div-", "tie")]
        for ci, (ha, va) in enumerate(combos):
            for qi, (sx, sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))):
                if (ha, va) == ("tie", "tie") and (sx, sy) == (-1, -1):
                    sx, sy = 1, 1      # both axes tying towards the centre would make the centre's raw cost the minimum: its discount wins
                beta = T * (5 if (ci + qi) % 2 else 10) // 4      # winner below / above 2T: BDOF off / on by the WINNER's cost
                mA, mB = -(-beta // (2 * cu)), -(-beta // (2 * cv))
                beta = cu * mA + cv * mB
                dA, dB = -(-beta // (2 * cu)) + 1, -(-beta // (2 * cv)) + 1
                steps = {"div+": (3, 1), "div-": (1, 3), "tie": (2, 0)}
                A = _valley(sx, mA, steps[ha][0] * dA, steps[ha][1] * dA, 2 * dA)
                B = _valley(sy, mB, steps[va][0] * dB, steps[va][1] * dB, 2 * dB)
                specs.append(_spec(w, h, ("off", (sx, sy), ha, va, beta), additive_windows(w, h, bd, A, B)))
        # -- the centre stays best: a neighbour ties its DISCOUNTED cost (-8 / +8 / both: zero denominator), or is between it and the raw cost
        for axis in (0, 1):
            unit = cu if axis == 0 else cv      # cost of one sample-sum unit on the axis under test
            other = cv if axis == 0 else cu
            for kind in ("minus8", "plus8", "zero", "stay", "move"):
                for inst in range(4):
                    thr = T if inst < 2 else 2 * T
                    n = max(4, -(-thr // (3 * unit)) + 1)      # discounted centre 3 * n * unit: >= T (searched), inst >= 2: >= 2T
                    e = 1
                    near = {"minus8": (3 * n, 3 * n + e), "plus8": (3 * n + e, 3 * n), "zero": (3 * n, 3 * n), "stay": (3 * n + e, 3 * n + 2 * e),
                            "move": (3 * n + 2 * e, 3 * n - e)}[kind]
                    X = [near[0] + 2 * n, near[0], 4 * n, near[1], near[1] + 2 * n]
                    yb = -(-4 * n * unit // other)      # the other axis: a lopsided pair far above, so its parabola gives a nonzero division result
                    ys = (yb, 1) if inst % 2 == 0 else (1, yb)
                    Y = [ys[0] + yb, ys[0], 0, ys[1], ys[1] + yb]
                    A, B = (X, Y) if axis == 0 else (Y, X)
                    specs.append(_spec(w, h, ("ctr", axis, kind, "+" if inst % 2 == 0 else "-", 4 * n * unit), additive_windows(w, h, bd, A, B)))
    # -- one 32 x 32 PU whose sub-PUs move differently: columns [tie +8 | edge], rows [division + | division -]
    w = h = 16
    cu, cv = sc * 8, sc * 16
    beta = 10 * 256 // 4
    m = -(-beta // (2 * cu))
    d = m + 1
    a = [0] * 36
    a[0] = d                                   # left sub-PUs: A = [m + d, m, m, m, m]: winner -1 ties its right neighbour
    for i in range(12):
        a[4 + i] = m // 12 + (i < m % 12)
    for i in range(12):
        a[20 + i] = m // 12 + (i < m % 12)     # right sub-PUs: A = [m, m + d, m + 2d, ...]: winner -2, on the border
    a[32:36] = [d, d, d, d]
    mb = -(-beta // (2 * cv))
    db = mb + 1
    b = [0] * 36
    # upper sub-PUs: odd rows B(-1) = mb + db, B(1) = mb; even rows B(-2) = B(0) = mb + 3 db, B(2) = mb + db  -> winner oy = +1, division +
    up_even, up_odd = slide([mb + 3 * db, mb + 3 * db, mb + db], 8), slide([mb + db, mb], 8)
    # lower sub-PUs: odd rows B(-1) = mb, B(1) = mb + db; even rows B(-2) = mb + db, B(0) = B(2) = mb + 3 db  -> winner oy = -1, division -
    lo_even, lo_odd = slide([mb + db, mb + 3 * db, mb + 3 * db], 8), slide([mb, mb + db], 8)
    assert up_even[8:] == [0, 0] and up_odd[8:] == [0] and lo_even[:2] == [0, 0] and lo_odd[:1] == [0]      # the rows the halves share stay 0
    b[0:20:2], b[1:18:2] = up_even, up_odd
    lo = [0] * 20
    lo[0::2], lo[1:18:2] = lo_even, lo_odd
    for i in range(20):
        b[16 + i] += lo[i]
    quad = (("off", (-1, 1), "tie", "div+"), ("edge", (-2, 1)), ("off", (-1, -1), "tie", "div-"), ("edge", (-2, -1)))
    specs.append(_spec(32, 32, ("quad", quad), profile_windows(32, 32, bd, a, b)))
    return specs


def clip_specs(bd):
    """Tie and threshold jobs whose vectors sit ON the clipMv bounds of a picture corner, so the refined vector crosses them: the window offset dX / dY comes
    from the unclipped vector, the phase from the clipped one."""
    specs = []
    ties = [s for s in tie_specs(bd) if s["label"][0] == "off"]
    thr = [s for s in threshold_specs(bd) if s["label"][0] == "winner"]
    for s in ties + thr:
        w, h = s["w"], s["h"]
        o = s["label"][1] if s["label"][0] == "off" else s["label"][3]
        if o[0] == 0 or o[1] == 0 or o[0] * o[1] < 0:
            continue
        if o[0] > 0:      # list 0 at the bottom-right bound, list 1 at the top-left one
            x, y = PIC_W - w, PIC_H - h
            mv = ((PIC_W + 7 - x) << 4, (PIC_H + 7 - y) << 4, (-CTU - 7 - x) << 4, (-CTU - 7 - y) << 4)
        else:
            x, y = 0, 0
            mv = ((-CTU - 7 - x) << 4, (-CTU - 7 - y) << 4, (PIC_W + 7 - x) << 4, (PIC_H + 7 - y) << 4)
        assert clip_mv(mv[0], mv[1], x, y) == mv[:2] and clip_mv(mv[2], mv[3], x, y) == mv[2:]
        specs.append(dict(s, mv=mv, pos=(x, y)))
    return specs


# ---------------------------------------------------------------------------------------------------------------- DMVR tables
class DmvrTable:
    def __init__(self, name, bd, specs):
        self.name, self.bd, self.specs, self.n = name, bd, specs, len(specs)
        k0 = {"thr": 0, "tie": 1, "clip": 2}[name]
        self.org = hash_tex(PIC_H, PIC_W, 7 + k0, 1 << (bd - 1), 1, 1 << (bd - 2))
        self.orgc = [hash_tex(PIC_H // 2, PIC_W // 2, 11 + c + k0, 1 << (bd - 1), 1, 1 << (bd - 2)) for c in range(2)]
        luma, chroma, at, atc = [np.zeros(HEAD, np.int16)], [np.zeros(HEAD, np.int16)], HEAD, HEAD
        self.jobs = []
        for k, s in enumerate(specs):
            w, h = s["w"], s["h"]
            x, y = s["pos"] if s["pos"] else ((k * 24) % (PIC_W - w + 1) & ~7, (k * 40) % (PIC_H - h + 1) & ~7)
            mv = s["mv"] if s["mv"] else (16 * (k % 5 - 2), 16 * (k % 3 - 1), 16 * ((k // 2) % 5 - 2), 16 * ((k // 3) % 3 - 1))
            S, Sc = w + 7 + 2 * GUARD, w // 2 + 3 + 2 * GUARD
            off, offc = [0, 0], [[0, 0], [0, 0]]
            for l in range(2):
                ph, pv = clip_mv(mv[2 * l] - 48, mv[2 * l + 1] - 48, x, y)
                tile = np.pad(s["win"][l], GUARD, mode="edge")
                assert tile.shape == (h + 7 + 2 * GUARD, S) and tile.min() >= 0 and tile.max() < (1 << bd)
                off[l] = at + (GUARD - (pv >> 4)) * S + GUARD - (ph >> 4)
                luma.append(tile.reshape(-1))
                at += tile.size
                pc, pvc = clip_mv(mv[2 * l] - 32, mv[2 * l + 1] - 32, x, y)
                for c in range(2):
                    tile = hash_tex(h // 2 + 3 + 2 * GUARD, Sc, 1000 + 4 * k + 2 * l + c, 1 << bd, 1, 0)
                    offc[c][l] = atc + (GUARD - (pvc >> 5)) * Sc + GUARD - (pc >> 5)
                    chroma.append(tile.reshape(-1))
                    atc += tile.size
            self.jobs.append(dict(w=w, h=h, x=x, y=y, mv=mv, S=S, Sc=Sc, off=off, offc=offc, bio=(0, 1, 1, 0)[k % 4], label=s["label"],
                                  nsub=(w // min(w, 16)) * (h // min(h, 16))))
        luma.append(np.zeros(HEAD, np.int16))
        chroma.append(np.zeros(HEAD, np.int16))
        self.refs, self.crefs = np.ascontiguousarray(np.concatenate(luma)), np.ascontiguousarray(np.concatenate(chroma))

    def luma_origin(self, k, l):
        """Address of sample (0, 0) of the virtual reference picture of job k, list l (only the job's window exists)."""
        j = self.jobs[k]
        return C.c_void_p(self.refs.ctypes.data + 2 * (j["off"][l] - (j["y"] * j["S"] + j["x"])))

    def chroma_origin(self, k, l, c):
        j = self.jobs[k]
        return C.c_void_p(self.crefs.ctypes.data + 2 * (j["offc"][c][l] - ((j["y"] // 2) * j["Sc"] + j["x"] // 2)))

    def expect(self):
        """Oracle results of every job, once: pred, mvd [n][4][2], per-sub-PU traces, chroma preds [n][2], BDOF counts."""
        if not hasattr(self, "_exp"):
            L = ol.oracle()
            pred, mvds, traces, cpred, bt = [], np.zeros((self.n, 4, 2), np.int32), [], [], ol.BdofTrace()
            for k, j in enumerate(self.jobs):
                w, h = j["w"], j["h"]
                e, mvd, tr = np.zeros((h, w), np.int16), np.zeros(2 * j["nsub"], np.int32), (ol.DmvrTrace * j["nsub"])()
                L.vo_dmvr_pu_ex(self.luma_origin(k, 0), self.luma_origin(k, 1), j["S"], PIC_W, PIC_H, CTU, j["x"], j["y"], w, h, *j["mv"], self.bd, j["bio"],
                                ol.P(e), w, ol.P(mvd), tr, C.byref(bt))
                pred.append(e)
                mvds[k, :j["nsub"]] = mvd.reshape(-1, 2)
                traces.append(tr)
                cc = []
                for c in range(2):
                    ec = np.zeros((h // 2, w // 2), np.int16)
                    L.vo_dmvr_chroma(self.chroma_origin(k, 0, c), self.chroma_origin(k, 1, c), j["Sc"], PIC_W, PIC_H, CTU, j["x"], j["y"], w, h, *j["mv"],
                                     ol.P(mvd), self.bd, ol.P(ec), w // 2)
                    cc.append(ec)
                cpred.append(cc)
            self._exp = dict(pred=pred, mvd=mvds, trace=traces, cpred=cpred, bdof=bt)
        return self._exp


@functools.lru_cache(maxsize=None)
def dmvr_table(name, bd):
    return DmvrTable(name, bd, {"thr": threshold_specs, "tie": tie_specs, "clip": clip_specs}[name](bd))


DMVR_TABLES = ("thr", "tie", "clip")


# ---------------------------------------------------------------------------------------------------------------- DMVR census
def _surf_sign(trace, mvd, axis):
    """'+', '-' or '0': the division result the error surface added on the axis."""
    whole = ((trace.best % 5 - 2), (trace.best // 5 - 2))[axis] * 16
    d = int(mvd[axis]) - whole
    return "+" if d > 0 else "-" if d < 0 else "0"


def classify(j, s, trace, mvd, label, bd):
    """The census classes sub-PU s of job j is IN, by the oracle's trace; asserts the ones its label promises."""
    dx, dy = min(16, j["w"]), min(16, j["h"])
    T, cost, best = dx * dy, list(trace.cost), trace.best
    got = set()
    ctx = (j["w"], j["h"], label, best, cost, list(mvd), list(trace.surface))
    names = {ol.SURF_ZERO_DENOM: "zero", ol.SURF_DIV: "div", ol.SURF_MINUS8: "minus8", ol.SURF_PLUS8: "plus8"}
    for axis in (0, 1):
        sf = trace.surface[axis]
        if sf in names:
            got.add("%s_%s" % (names[sf], "hv"[axis]))
            if sf == ol.SURF_DIV and _surf_sign(trace, mvd, axis) != "0":
                got.add("div%s_%s" % (_surf_sign(trace, mvd, axis), "hv"[axis]))
    if trace.surface[0] == ol.SURF_EDGE:
        got.add("edge_skip")
    if trace.notZero:
        mn = min(cost)
        firsts = [i for i in range(25) if cost[i] == mn]
        assert best == (12 if cost[12] == mn else firsts[0]), ctx      # the centre starts as the minimum; after it, raster order decides
        if len(firsts) > 1 and best != 12 and firsts[1] != 12:
            got.add("tie_same_row" if firsts[1] // 5 == best // 5 else "tie_rows")
    if label[0] == "centre":
        _, name, val = label
        assert cost[12] == val and best == 12, ctx
        assert trace.notZero == (val >= T) and trace.bio == (j["bio"] if val >= 2 * T else 0), ctx
        if trace.notZero:
            assert min(c for i, c in enumerate(cost) if i != 12) > 4 * T, ctx
        exact = {"T-": T - 1, "T": T, "2T-": 2 * T - 1, "2T": 2 * T}[name]
        assert val == exact or bd == 8, ctx
        assert (val < exact + 1) if name.endswith("-") else (val >= exact), ctx
        got.add("centre_" + name)
        if val == exact:
            got.add("exact_centre_" + name)
    elif label[0] == "centre_moves":
        _, val, axis, side = label
        assert cost[12] == val and trace.notZero and best == 12 + side * (1, 5)[axis] and cost[best] < T and not trace.bio, ctx
        got.add("centre_T_moves")
        if val == T:
            got.add("exact_centre_T_moves")
    elif label[0] == "winner":
        _, name, val, o = label
        assert best == (o[1] + 2) * 5 + o[0] + 2 and cost[best] == val and trace.bio == (j["bio"] if val >= 2 * T else 0), ctx
        assert (trace.surface[0] == ol.SURF_EDGE) == (2 in (abs(o[0]), abs(o[1]))), ctx
        assert sorted(cost)[1] > 4 * T and cost[12] > 4 * T, ctx
        got.add("winner_" + name)
        if val == {"2T-": 2 * T - 1, "2T": 2 * T}[name]:
            got.add("exact_winner_" + name)
    elif label[0] == "off":
        (sx, sy), ha, va = label[1], label[2], label[3]
        assert best == (sy + 2) * 5 + sx + 2, ctx
        for axis, a in ((0, ha), (1, va)):
            if a == "tie":
                assert trace.surface[axis] == ol.SURF_PLUS8 and cost[best + (1, 5)[axis]] == cost[best], ctx
            else:
                assert trace.surface[axis] == ol.SURF_DIV and _surf_sign(trace, mvd, axis) == a[3], ctx
        if trace.bio != j["bio"]:
            assert cost[best] < 2 * T, ctx
            if cost[12] >= 2 * T:
                got.add("bio_off_by_winner_only")
    elif label[0] == "edge":
        o = label[1]
        assert best == (o[1] + 2) * 5 + o[0] + 2 and trace.surface[0] == ol.SURF_EDGE, ctx
    elif label[0] == "ctr":
        _, axis, kind, sign, raw = label
        nb = (1, 5)[axis]
        if kind == "move":
            assert best == 12 + nb and cost[best] < cost[12] and trace.surface[axis] == ol.SURF_DIV, ctx
            got.add("disc_move")
        else:
            assert best == 12 and trace.notZero, ctx
            want = {"minus8": ol.SURF_MINUS8, "plus8": ol.SURF_PLUS8, "zero": ol.SURF_ZERO_DENOM, "stay": ol.SURF_DIV}[kind]
            assert trace.surface[axis] == want, ctx
            assert trace.surface[1 - axis] == ol.SURF_DIV and _surf_sign(trace, mvd, 1 - axis) == sign, ctx
            if kind == "stay":
                assert cost[12] < cost[12 - nb] < raw and cost[12] < cost[12 + nb] < raw, ctx      # only the discount keeps the centre
                got.add("disc_stay")
            if kind in ("minus8", "zero"):
                assert cost[12 - nb] == cost[12], ctx
            if kind in ("plus8", "zero"):
                assert cost[12 + nb] == cost[12], ctx
    for l in range(2):      # the refined vector beyond clipMv
        sg = -1 if l else 1
        rh, rv = j["mv"][2 * l] + sg * int(mvd[0]), j["mv"][2 * l + 1] + sg * int(mvd[1])
        sxp, syp = j["x"] + 16 * (s % (j["w"] // dx)), j["y"] + 16 * (s // (j["w"] // dx))
        if clip_mv(rh, rv, sxp, syp) != (rh, rv) and ((rh & 15) or (rv & 15)):
            got.add("clip_changes_phase")
    return got


def dmvr_census(tab):
    """{ (dx, dy): { class: count } } over the sub-PUs of a table; asserts every label on the way."""
    exp, out = tab.expect(), {}
    for k, j in enumerate(tab.jobs):
        labels = j["label"][1] if j["label"][0] == "quad" else (j["label"],)
        assert len(labels) == j["nsub"]
        seen = []
        for s in range(j["nsub"]):
            cls = classify(j, s, exp["trace"][k][s], exp["mvd"][k, s], labels[s], tab.bd)
            cell = out.setdefault((min(16, j["w"]), min(16, j["h"]), j["w"] > 16), {})
            for c in cls:
                cell[c] = cell.get(c, 0) + 1
            seen.append(tuple(exp["mvd"][k, s]))
        if j["label"][0] == "quad" and tab.name == "tie":
            assert len(set(seen)) == 4, seen      # four different vector differences: a wrong sub-PU index shows
    return out


# ---------------------------------------------------------------------------------------------------------------- BDOF tables
PHASES = ((0, 0, 0, 0), (8, 8, 8, 8), (0, 8, 8, 0), (4, 12, 0, 8), (3, 0, 13, 5), (8, 0, 0, 0), (0, 0, 0, 8))


def _stripes(h, w, bd, anti, lo, hi, phase):
    y, x = np.mgrid[0:h, 0:w]
    g = np.array([lo, hi, hi, lo])
    return g[((x - y if anti else x + y) + phase) & 3].astype(np.int16)


def _smooth(h, w, bd, x0, y0):
    """A slowly varying surface: a quadratic in the picture position, well inside the range."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    x, y = x + x0, y + y0
    v = (1 << (bd - 2)) + ((((x - 20) * (x - 20) * 3 + (y - 14) * (y - 14) * 2 + (x - 20) * (y - 14) * 2) << (bd - 8)) >> 8)
    return np.clip(v, 0, (1 << bd) - 1).astype(np.int16)


def _wave(h, w, bd, vertical, lo, hi, phase):
    y, x = np.mgrid[0:h, 0:w]
    t = ((y if vertical else x) + phase) % 6
    tri = np.array([0, 1, 3, 4, 3, 1])[t]
    return (lo + (hi - lo) * tri // 4).astype(np.int16)


def bdof_specs(bd):
    """(w, h, group, mv, tile0, tile1): tiles are (h+8) x (w+8), their origin 4 samples up-left of the whole-sample part of the vector."""
    mx = (1 << bd) - 1
    specs = []
    for (w, h) in SHAPES + ((32, 32),):
        th, tw = h + 8, w + 8
        phases = PHASES if w < 32 else PHASES[3:5]
        for pi, fr in enumerate(phases):
            whole = (16 * (pi % 3 - 1), 16 * ((pi // 2) % 3 - 1), 16 * ((pi + 1) % 3 - 1), 16 * (pi % 2))
            mv = tuple(a + b for a, b in zip(whole, fr))
            for anti in (0, 1):      # diagonal stripes over the full range; list 1 weaker or a phase later, so tmpx != 0
                specs.append((w, h, "anti" if anti else "diag", mv, _stripes(th, tw, bd, anti, 0, mx, 0), _stripes(th, tw, bd, anti, mx // 4, mx - mx // 4, 0)))
                specs.append((w, h, "anti" if anti else "diag", mv, _stripes(th, tw, bd, anti, 0, mx, 0), _stripes(th, tw, bd, anti, mx // 8, mx - mx // 3, 1)))
            # one plane, vectors less than a sample apart
            x0, y0 = 8 * pi, 5 * pi
            near = (mv[0], mv[1], mv[0] + (5, -7, 11, -3, 9, 2, -13)[pi], mv[1] + (-6, 4, 3, -12, 1, 14, -2)[pi])
            specs.append((w, h, "close", near, _smooth(th, tw, bd, x0 + (near[0] >> 4), y0 + (near[1] >> 4)), _smooth(th, tw, bd, x0 + (near[2] >> 4), y0 + (near[3] >> 4))))
            for vertical in (0, 1):      # columns only / rows only: one gradient sum is 0
                specs.append((w, h, "rows" if vertical else "cols", mv, _wave(th, tw, bd, vertical, mx // 4, mx // 2, 0), _wave(th, tw, bd, vertical, mx // 4, mx - mx // 4, 1 + pi % 2)))
            # within 3 of either end of the range, against steps into the range: the 8-tap overshoot and the refinement cross 0 / the maximum
            specs.append((w, h, "low", mv, _stripes(th, tw, bd, pi % 2, pi % 4, mx // 2, 0), _wave(th, tw, bd, pi % 2, 3 - pi % 4, mx // 3, 2)))
            specs.append((w, h, "high", mv, _stripes(th, tw, bd, pi % 2, mx - pi % 4, mx // 2, 0), _wave(th, tw, bd, pi % 2, mx - 3 + pi % 4, mx - mx // 3, 2)))
    return specs


class BdofTable:
    def __init__(self, bd):
        self.bd, self.specs = bd, bdof_specs(bd)
        self.n = len(self.specs)
        self.org = hash_tex(PIC_H, PIC_W, 5, 1 << (bd - 1), 1, 1 << (bd - 2))
        parts, at, self.jobs = [np.zeros(HEAD, np.int16)], HEAD, []
        for k, (w, h, group, mv, t0, t1) in enumerate(self.specs):
            S, off = w + 8, [0, 0]
            for l, t in enumerate((t0, t1)):
                assert t.shape == (h + 8, S) and t.min() >= 0 and t.max() < (1 << bd)
                off[l] = at + (4 - (mv[2 * l + 1] >> 4)) * S + 4 - (mv[2 * l] >> 4)
                parts.append(t.reshape(-1))
                at += t.size
            self.jobs.append(dict(w=w, h=h, group=group, mv=mv, S=S, off=off, x=(k * 24) % (PIC_W - w + 1) & ~3, y=(k * 40) % (PIC_H - h + 1) & ~3))
        parts.append(np.zeros(HEAD, np.int16))
        self.refs = np.ascontiguousarray(np.concatenate(parts))

    def expect(self):
        """pred per job and the BDOF counts per (shape, group)."""
        if not hasattr(self, "_exp"):
            L, pred, counts = ol.oracle(), [], {}
            for j in self.jobs:
                w, h = j["w"], j["h"]
                e, tr = np.zeros((h, w), np.int16), ol.BdofTrace()
                at = [C.c_void_p(self.refs.ctypes.data + 2 * j["off"][l]) for l in range(2)]
                L.vo_bdof_pu_ex(at[0], j["S"], at[1], j["S"], w, h, *j["mv"], self.bd, ol.P(e), w, C.byref(tr))
                pred.append(e)
                counts.setdefault((w, h, j["group"]), ol.BdofTrace()).add(tr)
            self._exp = dict(pred=pred, counts=counts)
        return self._exp


@functools.lru_cache(maxsize=None)
def bdof_table(bd):
    return BdofTable(bd)
