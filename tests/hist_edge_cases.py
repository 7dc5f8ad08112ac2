"""Inputs and plain NumPy expectations for the bin-edge sweep of the type-2 positional histogram (State.
add_positional_dist_type == 2, network.py:473-513 over dist_piggy, network.py:538-558) with the viewers OFF the origin -
no GPU needed.  The older sweep (tests/test_gpu_edges.py) keeps every viewer at post-move x == 0; the kernels fold the
viewer's own post-move position npx into their bin arithmetic in three different ways (step_fast64_body.inc `column`,
`column32` / `band32`; step_wide_closure.inc's one-fma form), and that sweep checks the fold-in only where it is zero.

One case per row (path, K, rb, L, N, lanes), B = 3 envs, valid for import_state on every table form:

* communication range 0: nobody hears anybody, the imported tables reach the histogram only stamped and aged;
* own positions: the viewers with equal u % 6 share one post-move position - six per env: 0, the midpoint of two
  float32 neighbours near L / 3 (its float32 conversion loses exactly half a float32 ulp), L / 2 + a dyadic offset, a
  full-mantissa value in (0.6 L, 0.7 L), L - rb / 3 floored to an eighth, and the largest position below L that a move
  reaches.  The vehicles move: npx = (px + vel + L) % L on float64 as the reference does (network.py:194-199);
  tests/test_hist_edge_cases.py asserts that the oracle's exported pos_x after the step IS that npx;
* stamps: viewer u holds the stamp of lag lag[u][k] about subject k; all viewers that hold one (subject, lag) stamp
  share u % 6, so the stamp is aimed at their position: fl(npx + e) for an interior edge e, and the float64 neighbour
  that puts x - npx nearest below / above e; targets at -rb and +rb (the reference's d < Rb decides) and one step
  inside; npx itself (v == +0), and from the position 0 the values 5e-324 and 1e-300 (the kernels' |v| < 2^-500
  branch) and -0.0; walks of up to three steps around random edges; edges of the SECOND slot's position (the K-slot
  launches of a rollout); uniform random values.  Targets outside [0, L] are replaced by uniform ones;
* quad forms: the kernels split the subjects at multiples of 4 (step_fast64_body.inc: `const int c = 4 * q + cc`, the
  test `rare` at its "a byte with (code & 0x7f) == 0" line decides per quad between the straight-line fast body and
  the column loop `tally`; step_wide_closure.inc: `rare` / `slowq` in front of the one-fma loop).  Quad k // 4 of env
  b has form FORMS[(k // 4 + b) % 5]:
    fast     every viewer's entry lags its subject by 0 ... 5 at the import, 1 ... 6 behind the slot's stamp: the
             fast quad (lag 0 is the subject's current stamp, its xpos the subject's own position);
    handover lags 1 ... 6 at the import: the entries of lag 6 reach lag 7 under the stamp (code 0x80) - the column
             loop, and the hand-over to the planes;
    ghost    some viewers hold a never-heard entry (sequence number 0) of age <= 18, an aimed value as its ghost xpos -
             one value per subject, aimed at the first of those viewers: equal sequence numbers, 0 included, carry equal
             xpos (step_wide's plane form keeps one xpos per subject and rank) -: the column loop, FLAT branch of `tally`
             with the xpos from the plane;
    oldghost the same with ages 19 (20 under the stamp: the limit), 25 and 200: the column loop, nothing counted;
    beyond   lag 9 at the import in place of lag 5: beyond the ring, the keyed path of step_fast64 (`badq`), the slow
             quad of step_wide.
  Which path a quad takes cannot be observed from outside; it follows from those lines by construction;
* 2-D rows (lanes == 2): the vehicles alternate between y = 0 and y = 60; a stamp whose subject is on the other lane
  is aimed at dx = +-80 (and one float64 step either side): sqrt(80^2 + 60^2) is exactly 100, an edge of (K, rb) =
  (10, 500) and (20, 500) - with dy = 60 the only edge of the rows here that a Pythagorean triple reaches (80 j gives
  100 j only beside dy = 60 j) -, and at every edge |e| > 60 through the stamps around dx = +-sqrt(e^2 - 60^2) whose
  value falls nearest below / above e or, where the square root rounds that way, on it; same-lane pairs as above.

`expected` is the statement of the reference itself, per viewer np.histogram(sorted(vals), K, range=(-rb, rb))[0] /
len(vals).  `f32_model_t16` is a NumPy MODEL of the float32 screen of step_fast64 - the fma taken as a float64 product
and sum rounded once to float32, which may differ from the hardware's v_fma_f32 in the last bit - and is used for
existence conditions only (do the inputs reach into the band?), never to predict a kernel's output."""
import collections
import functools
import math

import numpy as np

from diral_amd.config import bench_config

A = 4
B = 3
AGE_LIMIT = 20                                   # an entry of age >= 20 is not used (dist_piggy, network.py:547)
T0 = 50                                          # every subject's own sequence number at the import
NTYPES = 6
SPEEDS = (1.5, 2.25, 1.25, 2.5, 1.75, 2.0)       # by position type: dyadic, inside the reference's 1.1 ... 2.77
HIGH_TYPES = (2, 3, 4, 5)                        # the position types with npx >= L / 2; type 0 is npx == 0
FORMS = ("fast", "handover", "ghost", "oldghost", "beyond")
YOUNG_AGES, OLD_AGES = (18, 5, 17, 0), (19, 25, 19, 200)
LANE_Y = 60.0
UNDERFLOW_STAMPS = (5e-324, 1e-300, -0.0)       # from the position 0: the |v| < 2^-500 branch, and v == -0

KRB = [(10, 500.0), (20, 500.0), (40, 500.0), (20, 123.456), (7, 250.0), (64, 500.0)]
# where the host leaves the float32 screening of step_fast64 ON (csrc/diral_env.hip f32_margin16: a band of at most 64
# units of 2^-16 bin widths, L < 1e6), as a list: every (K, rb) at L = 2000, these beyond.  Whether the screening is on
# cannot be observed from outside: the list MUST be derived again from f32_margin16 whenever that function changes, or
# the DIRAL_F32_MARGIN=0 reruns and the CPU existence test drift to the wrong rows without anything failing
SCREEN_ON = {2000.0: set(KRB), 131072.0: {(10, 500.0), (20, 500.0), (7, 250.0)}, 150000.0: {(10, 500.0), (7, 250.0)},
             1e6: set()}

Row = collections.namedtuple("Row", "path K rb L N lanes")


def _rows():
    rows = []
    for L in (2000.0, 131072.0, 150000.0, 1e6):
        rows += [Row("fast64", K, rb, L, N, 1) for N in (64, 40) for K, rb in KRB]
    for L in (2000.0, 131072.0):
        rows += [Row("fast64_y", K, rb, L, 64, 2) for K, rb in KRB]             # off y = 0: the non-FLAT instantiation
    for L in (2000.0, 131072.0, 2.0 ** 30):
        rows += [Row("wide", K, rb, L, N, 1) for N in (65, 128, 200, 256) for K, rb in KRB]
    for L in (2000.0, 131072.0):
        rows += [Row("general", K, rb, L, 64, 1) for K, rb in KRB]              # force_general_kernel
        rows += [Row("general", K, rb, L, 130, 2) for K, rb in KRB]             # two lanes beyond 64 vehicles
        rows += [Row("large", K, rb, L, 257, 1) for K, rb in KRB]               # N > 256
        rows += [Row("large", 65, rb, L, 100, 2) for K, rb in KRB if K == 64]   # K > 64
        rows += [Row("large", K, rb, L, 64, 1) for K, rb in KRB]                # force_large_path
    return rows


ROWS = _rows()


def row_id(r):
    return "%s-K%d-rb%g-L%g-N%d%s" % (r.path, r.K, r.rb, r.L, r.N, "-2lanes" if r.lanes == 2 else "")


def screening_on(r):
    return r.path == "fast64" and (r.K, r.rb) in SCREEN_ON[r.L]


def config(r):
    return bench_config(r.N, A, r.L, bin_range=r.rb, communication_range=0.0, State=dict(num_bins=r.K))


def move(px, vel, L):
    """update_positions (network.py:194-199) on float64, element by element in Python's own arithmetic."""
    px, vel = np.asarray(px, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    out = np.empty(px.shape)
    for i in np.ndindex(px.shape):
        out[i] = (float(px[i]) + float(vel[i]) + L) % L
    return out


def _steps1(x, n):
    """One float64 moved by n steps (math.nextafter: no array round trip)."""
    x = float(x)
    for _ in range(abs(int(n))):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def _own_positions(r, rng):
    """px, npx [B][type]: the pre-move position whose move lands on (or, for the last type, nearest below) the target."""
    L, rb = r.L, r.rb
    px, npx = np.empty((B, NTYPES)), np.empty((B, NTYPES))
    for b in range(B):
        m = np.float32(L / 3.0 + 11.0 * b)
        targets = [0.0, float(m) + 0.5 * float(np.spacing(m)), L / 2.0 + 0.375 * b, float(rng.uniform(0.6 * L, 0.7 * L)),
                   np.floor((L - rb / 3.0) * 8.0) / 8.0 - 0.125 * b, float(np.nextafter(L, 0.0))]
        for p, T in enumerate(targets):
            v = SPEEDS[p]
            if p == 0:
                cands = [L - v]
            elif p == NTYPES - 1:
                cands = [_steps1(L - v, -i) for i in range(0, 4)] + [L - v - 2.0 ** -20 * L]
            else:
                cands = [T - v]
            best = max(cands, key=lambda c: ((c + v + L) % L) if p else -((c + v + L) % L))
            px[b, p], npx[b, p] = best, (best + v + L) % L
    assert (px >= 0).all() and (px <= L).all() and (npx >= 0).all() and (npx < L).all()
    assert (npx[:, 0] == 0).all() and (npx[:, list(HIGH_TYPES)] >= L / 2).all() and (npx[:, 5] > L - 2.0 ** -19 * L).all()
    return px, npx


def grid_step(npx, e):
    """The step of the grid a stamp aimed from npx at the value e moves on."""
    return np.spacing(np.abs(npx + e))


def where_about(v, e, g):
    """0: v on e; -1 / +1: within one grid step g below / above it; 9: elsewhere."""
    return 0 if v == e else -1 if (v < e and e - v <= g) else 1 if (v > e and v - e <= g) else 9


def _value(x, npx, dy):
    dx = float(x) - float(npx)
    d = math.sqrt(dx * dx + dy * dy)
    return d if dx > 0 else -d


def _pick(npx, e, kind, dy=0.0):
    """The stamp aimed from npx at the edge e, or None: kind 0 the one whose value is e, else fl(npx + e); -1 / +1 the
    float64 neighbour whose value is the nearest below / above e, within one grid step.  dy != 0: the subject is on the
    other lane, the value is +-sqrt(dx^2 + dy^2) and the stamp is searched around dx = +-sqrt(e^2 - dy^2)."""
    if dy != 0.0 and abs(e) <= abs(dy):
        return None
    x0 = npx + (e if dy == 0.0 else np.copysign(np.sqrt(e * e - dy * dy), e))
    c = [_steps1(x0, n) for n in (range(-1, 2) if dy == 0.0 else range(-3, 4))]
    v = [_value(x, npx, dy) for x in c]
    g = grid_step(npx, e)
    if kind == 0:
        hit = [x for x, w in zip(c, v) if w == e]
        return hit[0] if hit else (float(x0) if dy == 0.0 else None)
    ok = [(w, x) for x, w in zip(c, v) if where_about(w, e, g) == kind]
    if not ok:
        return None
    return max(ok)[1] if kind < 0 else min(ok)[1]


def _layout(r, rng, px, ptype, lane):
    """Lags, ghosts and ages of one row, no value aimed yet: (seq, age, x, filler, form, slots, old_slots).  x holds the own
    entries and the lag-0 entries (the subject's own position), NaN elsewhere.  slots: the places a value can be aimed
    into, (env, position type of the viewers, other-lane flag, quad form, viewers, subject) - one per (subject, lag) stamp,
    whose viewers share u % 6, and one per subject for the young never-heard entries; old_slots: the same for the
    never-heard entries past the age limit, which nothing counts."""
    N = r.N
    uu, kk = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")                # [viewer][subject]
    cross = lane[uu] != lane[kk]
    seq, age, x = np.empty((B, N, N), np.int32), np.empty((B, N, N), np.int32), np.full((B, N, N), np.nan)
    filler = np.zeros((B, N, N), bool)
    form = np.stack([(np.arange((N + 3) // 4) + b) % len(FORMS) for b in range(B)])
    ghost_sel = (uu + 2 * kk) % 7 == 0
    F = {name: i for i, name in enumerate(FORMS)}
    slots, old_slots = [], []
    for b in range(B):
        fk = form[b][kk // 4]                                                       # [viewer][subject]
        lag = (uu + kk) % 6 + (fk == F["handover"])
        lag = np.where((fk == F["beyond"]) & (lag == 5), 9, lag)
        ghost = ghost_sel & np.isin(fk, (F["ghost"], F["oldghost"])) & (uu != kk)
        seq[b] = np.where(ghost, 0, T0 - lag)
        age[b] = rng.integers(0, AGE_LIMIT, size=(N, N))                            # 19 -> 20 under the stamp: not used
        age[b] = np.where(ghost, np.where(fk == F["ghost"], np.array(YOUNG_AGES)[(uu + kk) % 4],
                                          np.array(OLD_AGES)[(uu + kk) % 4]), age[b])
        for k in range(N):
            f = int(form[b][k // 4])
            age[b, k, k], seq[b, k, k], x[b, k, k] = 0, T0, px[b, k]
            others = np.arange(N) != k
            for l in np.unique(lag[others & ~ghost[:, k], k]):
                us = np.flatnonzero((lag[:, k] == l) & others & ~ghost[:, k])
                if l == 0:                                                          # the subject's current stamp: its own position
                    x[b, us, k], filler[b, us, k] = px[b, k], True
                    continue
                assert (ptype[b, us] == ptype[b, us[0]]).all()
                slots.append((b, int(ptype[b, us[0]]), bool(cross[us[0], k]), f, us, k))
            us = np.flatnonzero(ghost[:, k])          # one ghost xpos per subject: sequence number 0 is a sequence number too
            if len(us):                               # (a never-heard entry's ypos is 0, whatever the subject's lane)
                (slots if f == F["ghost"] else old_slots).append((b, int(ptype[b, us[0]]), bool(lane[us[0]] != 0), f, us, k))
    return seq, age, x, filler, form, slots, old_slots


def _targets(r, interior):
    """What to aim at, as (mode, value, kind): every interior edge - on it, one step below, one above -; the range ends
    and one step inside, and v == 0; on the 2-D rows dx = +-80 and its neighbours (mode "tri": the value is 1.25 dx)."""
    edge_items = [("edge", e, kind) for e in interior for kind in (0, -1, 1)]
    other_items = [("end", -r.rb, 0), ("end", r.rb, 0), ("end", -r.rb, 1), ("end", r.rb, -1), ("end", 0.0, 0)]
    if r.lanes == 2:
        other_items += [("tri", s * 80.0, n) for s in (-1.0, 1.0) for n in (0, -1, 1)]
    return edge_items, other_items


class _Dealer:
    """Deals targets into the slots of a row.  A pool is the set of slots of one (other-lane flag, position type, env,
    quad form); a target goes into the least loaded pool that reaches it - for kind 0 one that hits the value exactly,
    where any does.  deck[pool] is the list of stamps dealt to it, in order."""

    def __init__(self, r, tnpx, slots):
        self.r, self.tnpx = r, tnpx
        self.pools = {}
        for b, p, other, f, us, k in slots:
            self.pools.setdefault((int(other), p, b, f), []).append((us, k))
        self.deck = {key: [] for key in self.pools}
        self.aimed = {}

    def aim(self, item, p, b, pool):
        """The stamp of this target from position type p of env b for a slot whose subject is on the viewer's lane (pool
        0) or on the other (1), or None."""
        key = (item, p, b, pool)
        if key not in self.aimed:
            mode, e, kind = item
            n = self.tnpx[b, p]
            if mode == "tri":
                xx = _steps1(n + e, kind) if pool == 1 else None
            elif mode == "end":
                xx = _pick(n, e, kind) if pool == 0 else None
            else:
                xx = _pick(n, e, kind, LANE_Y if pool == 1 else 0.0)
            self.aimed[key] = xx if xx is not None and 0.0 <= xx <= self.r.L else None
        return self.aimed[key]

    def assign(self, item, types, want, form=None, pool=None):
        """The target goes to `want` different position types of `types` (into quads of `form` / slots of `pool` only,
        where given); returns the types that took it."""
        done = set()
        for _ in range(want):
            cand = []
            for key, places in self.pools.items():
                kpool, p, b, f = key
                if p not in types or p in done or len(self.deck[key]) >= len(places):
                    continue
                if (form is not None and f != form) or (pool is not None and kpool != pool):
                    continue
                xx = self.aim(item, p, b, kpool)
                if xx is not None:
                    goal = item[1] * 1.25 if item[0] == "tri" else item[1]           # (3-4-5: dx = 80, the value 100)
                    hit = item[2] == 0 and _value(xx, self.tnpx[b, p], LANE_Y * kpool) == goal
                    cand.append((not hit, len(self.deck[key]) / len(places), key, xx))
            if not cand:
                break
            _, _, key, xx = min(cand)
            self.deck[key].append(xx)
            done.add(key[1])
        return done

    def high_reach(self, item):
        return len({p for p in HIGH_TYPES for b in range(B) if self.aim(item, p, b, 0) is not None})


def _deal(r, dealer, interior):
    """The order of the deal.  First what must not be crowded out: the underflow values and -0 from the position 0; per
    quad form one value on, one below and one above an edge e > 0 (on it: the position 0 reaches every such edge exactly);
    on the 2-D rows a value below and one above every edge beyond the lane distance, into other-lane slots.  Then every
    edge target to two position types at or beyond L / 2 - the most constrained first: the upper edges are out of reach
    from L - rb / 3 and from L -, to the position 0 and to the one near L / 3, wherever a stamp in [0, L] reaches it."""
    edge_items, other_items = _targets(r, interior)
    every = range(NTYPES)
    for xx in UNDERFLOW_STAMPS:
        key = min((k for k in dealer.pools if k[0] == 0 and k[1] == 0), key=lambda k: len(dealer.deck[k]) / len(dealer.pools[k]))
        dealer.deck[key].append(xx)
    positive = [e for e in interior if e > 0]
    taken = {}                                                        # target -> the position types that hold it already
    for f in range(len(FORMS)):
        for i, kind in enumerate((0, -1, 1)):
            item = ("edge", positive[(f + i) % len(positive)], kind)
            took = dealer.assign(item, every, 1, form=f, pool=0)
            assert len(took) == 1, (f, kind)
            taken.setdefault(item, set()).update(took)
    if r.lanes == 2:
        for e in interior:
            for kind in (-1, 1):
                if abs(e) > LANE_Y:
                    dealer.assign(("edge", e, kind), every, 1, pool=1)

    def rest(item, types, want):
        have = taken.get(item, set()) & set(types)
        dealer.assign(item, [p for p in types if p not in have], want - len(have))
    for item in sorted(edge_items, key=dealer.high_reach):
        rest(item, HIGH_TYPES, 2)
    for item in edge_items:
        rest(item, (0,), 1)
    for item in other_items:
        dealer.assign(item, HIGH_TYPES, 1)
        dealer.assign(item, (0,), 1)
    for item in edge_items + other_items:
        rest(item, (1,), 1)


def _fill_value(r, rng, interior, n1, n2, other_lane):
    """A value for a slot no target took, seen from the position n1 (n2: where the second slot leaves that viewer):
    (x, filler) - a walk of up to three steps around an edge of either position, else a uniform value (filler)."""
    roll = rng.random()
    if roll < 0.85:
        base = n1 if roll < 0.55 else n2
        e = interior[rng.integers(0, len(interior))] if len(interior) else 0.0
        if other_lane:
            j = int(rng.integers(1, 7))
            e = float(rng.choice([-1.0, 1.0])) * (80.0 * j if rng.random() < 0.7 or abs(e) <= LANE_Y
                                                  else np.sqrt(e * e - LANE_Y * LANE_Y))
        xx = _steps1(base + e, rng.integers(-3, 4))
        if 0.0 <= xx <= r.L:
            return xx, False
    return float(min(max(n1 + rng.uniform(-r.rb, r.rb), 0.0), r.L)), True


@functools.lru_cache(maxsize=None)
def tables(r):
    """The import of one row: dict(px, py, vel [B][N]; npx, npx2 [B][N]: where the first and the second step leave the
    vehicles; ptype [B][N]; seq, age, x [B][viewer][subject]; filler [B][viewer][subject]: uniform random values and the
    lag-0 entries, which are aimed at nothing; form [B][quad]; acts [2][B][N]; edges).  Three steps: the layout of lags
    and ages (_layout), the deal of the targets into its slots (_deal), values for the slots left (_fill_value)."""
    K, rb, L, N = r.K, r.rb, r.L, r.N
    rng = np.random.default_rng([K, int(rb * 1000), int(L) % (1 << 31), N, r.lanes, len(r.path)])
    edges = np.linspace(-rb, rb, K + 1)
    interior = edges[1:-1]
    tpx, tnpx = _own_positions(r, rng)
    lane = (np.arange(N) % 2) * (r.lanes == 2)
    ptype = np.stack([(np.arange(N) + b) % NTYPES for b in range(B)])
    px = np.take_along_axis(tpx, ptype, axis=1)
    vel = np.array(SPEEDS)[ptype]
    npx = move(px, vel, L)
    assert np.array_equal(npx, np.take_along_axis(tnpx, ptype, axis=1))
    npx2 = move(npx, vel, L)
    tnpx2 = move(tnpx, np.broadcast_to(np.array(SPEEDS), tnpx.shape), L)
    seq, age, x, filler, form, slots, old_slots = _layout(r, rng, px, ptype, lane)
    dealer = _Dealer(r, tnpx, slots)
    for places in dealer.pools.values():
        rng.shuffle(places)
    _deal(r, dealer, interior)
    required = np.zeros((B, N, N), bool)
    for (pool, p, b, f), places in dealer.pools.items():
        for i, (us, k) in enumerate(places):
            if i < len(dealer.deck[(pool, p, b, f)]):
                x[b, us, k] = dealer.deck[(pool, p, b, f)][i]
                required[b, us[0], k] = True
            else:
                x[b, us, k], filler[b, us, k] = _fill_value(r, rng, interior, tnpx[b, p], tnpx2[b, p], pool == 1)
    for b, p, other, f, us, k in old_slots:
        x[b, us, k], filler[b, us, k] = _fill_value(r, rng, interior, tnpx[b, p], tnpx2[b, p], other)
    # a dealt target is counted by at least one of its viewers (18 -> 19 under the stamp: the last age that counts)
    heard = seq > 0
    age = np.where(required & heard, np.minimum(age, AGE_LIMIT - 2), age)
    assert not np.isnan(x).any() and (x >= 0).all() and (x <= L).all()
    for b in range(B):                      # equal (subject, sequence number), equal xpos: the import contract
        for k in range(N):
            h = heard[b, :, k]
            for s in np.unique(seq[b, h, k]):
                assert len(np.unique(x[b, h & (seq[b, :, k] == s), k])) == 1, (b, k, s)
    acts = rng.integers(0, A, size=(2, B, N)).astype(np.int32)
    return dict(px=px, py=np.broadcast_to(lane * LANE_Y, (B, N)).copy(), vel=vel, npx=npx, npx2=npx2, ptype=ptype, seq=seq,
                age=age, x=x, filler=filler, form=form, acts=acts, edges=edges, lane=lane)


def entry_y(t):
    """The ypos the oracle's import takes: the subject's lane once heard, 0 in a fresh entry."""
    return np.where(t["seq"] > 0, t["py"][:, None, :], 0.0)


# ---- the plain statement ----------------------------------------------------------------------------------------------
def numpy_hist(dx, dy, ok, K, rb, closed_range=False):
    """One viewer's row, the statement of network.py:473-513 over dist_piggy (network.py:538-558): dx, dy [subjects] =
    entry - own post-move position, ok [subjects] = not the own entry and younger than the limit behind the step."""
    d = np.sqrt(dx * dx + dy * dy)                       # Network.dist (network.py:318-332): a tiny dx underflows to 0
    keep = ok & ((d <= rb) if closed_range else (d < rb))
    vals = np.where(dx > 0, d, -d)[keep]                 # dist_piggy's sign: + iff x1 - x2 > 0 (network.py:552-556)
    return np.histogram(sorted(vals), K, range=(-rb, rb))[0] / float(len(vals)) if len(vals) else np.zeros(K)


def values(r, t, slot=1, own_at_zero=False):
    """dx, dy, ok [B][viewer][subject] behind slot 1 or 2."""
    own = (t["npx"] if slot == 1 else t["npx2"])[:, :, None]
    dx = t["x"] - (0.0 if own_at_zero else own)
    dy = entry_y(t) - t["py"][:, :, None]
    ok = (t["age"] + slot < AGE_LIMIT) & ~np.eye(r.N, dtype=bool)[None]
    return dx, dy, ok


def expected(r, t, slot=1, closed_range=False, own_at_zero=False):
    """[B][N][K]: numpy_hist of every viewer."""
    dx, dy, ok = values(r, t, slot, own_at_zero)
    return np.stack([np.stack([numpy_hist(dx[b, u], dy[b, u], ok[b, u], r.K, r.rb, closed_range) for u in range(r.N)])
                     for b in range(B)])


def counted(r, t, slot=1):
    """(v, keep) [B][viewer][subject]: the signed values and which of them the reference counts."""
    dx, dy, ok = values(r, t, slot)
    d = np.sqrt(dx * dx + dy * dy)
    return np.where(dx > 0, d, -d), ok & (d < r.rb)


# ---- wrong restatements, and the model of the float32 screen --------------------------------------------------------------
def inv_width(r):
    return float(r.K) / (r.rb - (-r.rb))                 # the host's hist_inv_width (csrc/diral_env.hip)


def f32_model_t16(r, x, npx):
    """A MODEL of step_fast64's float32 screen, in units of 2^-16 bin widths: trunc(float32(float32(x) * float32(inv_w
    2^16) + float32((rb - npx) inv_w 2^16))), the product and the sum taken in float64 and rounded ONCE to float32.  It
    is a model of the v_fma_f32 and may differ from the hardware in the last bit; for existence conditions only."""
    f = np.float32
    a = f(inv_width(r) * 65536.0).astype(np.float64)
    c = ((r.rb - npx) * inv_width(r) * 65536.0).astype(f).astype(np.float64)
    return np.trunc((np.asarray(x).astype(f).astype(np.float64) * a + c).astype(f).astype(np.float64)).astype(np.int64)


def true_bins(r, v):
    """np.histogram's bin of values inside [-rb, rb): the last edge that is <= v."""
    return np.clip(np.searchsorted(np.linspace(-r.rb, r.rb, r.K + 1), v, "right") - 1, 0, r.K - 1)


def _rows_from_bins(r, bins, keep):
    out = np.zeros(keep.shape[:2] + (r.K,))
    for b in range(keep.shape[0]):
        for u in range(keep.shape[1]):
            n = int(keep[b, u].sum())
            if n:
                out[b, u] = np.bincount(bins[b, u][keep[b, u]], minlength=r.K) / float(n)
    return out


def wrong_floor_estimate(r, t):
    """WRONG on purpose: the bin as floor((v + rb) * inv_w) with no correction against the edges."""
    v, keep = counted(r, t)
    return _rows_from_bins(r, np.clip(np.floor((v + r.rb) * inv_width(r)).astype(np.int64), 0, r.K - 1), keep)


def wrong_right_closed(r, t):
    """WRONG on purpose: bins closed on the right - a value on an edge falls into the bin below."""
    v, keep = counted(r, t)
    return _rows_from_bins(r, np.clip(np.searchsorted(np.linspace(-r.rb, r.rb, r.K + 1), v, "left") - 1, 0, r.K - 1), keep)


def wrong_closed_range(r, t):
    """WRONG on purpose: d <= rb in place of d < rb."""
    return expected(r, t, closed_range=True)


def wrong_f32_no_band(r, t):
    """WRONG on purpose: the float32 model's integer part taken as the bin with no band around the integers."""
    v, keep = counted(r, t)
    t16 = f32_model_t16(r, t["x"], t["npx"][:, :, None])
    return _rows_from_bins(r, np.clip(t16 >> 16, 0, r.K - 1), keep)


def wrong_own_at_zero(r, t):
    """WRONG on purpose: the own position taken as 0."""
    return expected(r, t, own_at_zero=True)


# ---- the oracle's side, computed once per row and shared by the CPU and the GPU tests ----------------------------------
FOREIGN_EPISODE, FOREIGN_EPS = 3.0, 0.25


def foreign_args(r):
    """Arguments of a stand-alone obtain_state that no step produced: (actions, channel observation, rewards)."""
    cfg = config(r)
    rng = np.random.default_rng(1700 + r.K + r.N)
    return (rng.integers(0, A, size=(B, r.N)).astype(np.int32), rng.uniform(0.0, 300.0, size=(B, r.N, cfg.chobs_width)),
            rng.uniform(-3.0, 1.0, size=(B, r.N)))


EXPORT_KEYS = ("pos_x", "vel", "seq", "age", "x")


@functools.lru_cache(maxsize=None)
def oracle(r):
    """dict(rew1, state1: one my_step on the imported tables; foreign: a stand-alone obtain_state behind it; export1;
    rew2, state2, export2: a second my_step)."""
    from diral_amd.config import STEP_MY_STEP
    from oracle.oracle import SQ_IEEE, Oracle
    t, cfg = tables(r), config(r)
    fa, fc, fr = foreign_args(r)
    orc = Oracle(cfg, batch=B, sq_mode=SQ_IEEE, threads=4)
    orc.reset(t["px"], t["py"], t["vel"])
    orc.import_state(seq=t["seq"], age=t["age"], x=t["x"], y=entry_y(t))
    out = {}
    for slot in (1, 2):
        a = t["acts"][slot - 1]
        rew, chobs = orc.step(STEP_MY_STEP, a, slot - 1)
        out["rew%d" % slot], out["state%d" % slot] = rew, orc.obtain_state(a, chobs, rew)
        if slot == 1:
            out["foreign"] = orc.obtain_state(fa, fc, fr, FOREIGN_EPISODE, FOREIGN_EPS)
        e = orc.export()
        out["export%d" % slot] = {k: e[k] for k in EXPORT_KEYS}
    return out
