"""The split rollout's three-wave LDS protocol as data: the documented schedule
(the resource / interval table) as a generator of access records, and a
checker that proves from such records -- the model's, or the ones a probe build of the
kernel logged (csrc/internal.h, "split protocol probe") -- that no two waves conflict inside
a barrier interval and that every read sees the write it was meant to see.  Nothing here
depends on timing or on a device.

A record is one access of one wave to one slot of a shared resource:
  wave      0 the step wave, 1 / 2 the store waves of step parity 0 / 1
  seq       the wave's program-order index
  interval  the barrier interval: barrier 0 is the prologue barrier, interval k the code
            between barriers k and k + 1, the prologue itself interval -1
  site      the annotated source site (SITES)
  res, slot the resource (RESOURCES) and its slot
  tag       the step the data belongs to, -1 for none
  kind      "R", "W", "RMW", or "SHARE": a write to the wave's own part of a slot that
            several waves fill together (the prologue's disjoint row shares)
The checker is not specific to the split kernel: any barrier-phased protocol that logs
such records can use it (the generic rollout's deferred-fold ring is the next candidate).
"""
import collections

# the numbers of csrc/internal.h (test_split_protocol.py compares them with the header)
RESOURCES = ("MAP", "INFO", "EDGE", "IMG", "CODE", "RTAB", "STAGE")
KINDS = ("R", "W", "RMW", "SHARE")
SITES = ("MAP_BUILD", "STAGE_COMMIT", "MAP_INIT", "STAGE_FIRST", "MAP_RESET", "MAP_MOVE",
         "STAGE_NEXT", "EDGE_PREV", "INFO_W", "EDGE_LAST", "RTAB_W", "INFO_R", "MAP_R", "IMG_W",
         "IMG_R", "EDGE_R", "CODE_W", "FOLD")
STEP_SITES = SITES[:10]                       # the step wave's
STORE_SITES = SITES[:2] + SITES[10:]          # each store wave's
PROBE_CAP = 1024
STAGE_FLAGS = 64                              # STAGE slot of the flag bytes (rows: 0 .. 63)
STAGE_ROWS = 48                               # rows per staging pass: 16 per wave
STAGE_MAX_T = 64

Rec = collections.namedtuple("Rec", "wave seq interval site res slot tag kind")
Finding = collections.namedtuple("Finding", "rule res slot interval waves detail")

MUTATIONS = ("early_last_fold", "no_third_edge_slot", "single_info_slot", "map_early",
             "code_ring_16")


class _Wave:
    def __init__(self, role, out):
        self.role, self.seq, self.nbar, self.out = role, 0, 0, out

    def acc(self, site, res, slot, tag, kind):
        self.out.append(Rec(self.role, self.seq, self.nbar - 1, site, res, slot, tag, kind))
        self.seq += 1

    def barrier(self):
        self.nbar += 1


def barriers(T):
    """Barriers each of the three waves passes in a launch of T steps."""
    return (T + 2,) * 3


def model(T, staged, recounts=(), mutate=None):
    """The records of one workgroup in a launch of T >= 1 steps, in each wave's program
    order.  staged: the actions are staged in LDS (T <= 64); recounts: the steps s whose
    iteration starts with an autoreset re-count of map s & 1; mutate: one of MUTATIONS, a
    schedule that is wrong on purpose."""
    assert T >= 1 and (not staged or T <= STAGE_MAX_T)
    assert mutate is None or mutate in MUTATIONS, mutate
    recounts = set(recounts)
    out = []
    ring = 16 if mutate == "code_ring_16" else 32
    last_edge = (T - 1) & 1 if mutate == "no_third_edge_slot" else 2

    def prologue(w):
        w.acc("MAP_BUILD", "MAP", 0, -1, "SHARE")
        w.acc("MAP_BUILD", "MAP", 1, -1, "SHARE")
        if staged:
            w.acc("STAGE_COMMIT", "STAGE", STAGE_FLAGS, -1, "SHARE")
            for r in range(T):
                if r % STAGE_ROWS // 16 == w.role:
                    w.acc("STAGE_COMMIT", "STAGE", r, -1, "W")
        w.barrier()                                        # barrier 0

    # ---- the step wave ----
    w = _Wave(0, out)
    prologue(w)
    w.acc("MAP_INIT", "MAP", 0, -1, "RMW")
    w.acc("MAP_INIT", "MAP", 1, -1, "RMW")
    if staged:
        w.acc("STAGE_FIRST", "STAGE", STAGE_FLAGS, -1, "R")
        w.acc("STAGE_FIRST", "STAGE", 0, -1, "R")

    def move(s):
        if s in recounts:
            w.acc("MAP_RESET", "MAP", s & 1, s, "RMW")
        w.acc("MAP_MOVE", "MAP", s & 1, s, "RMW")

    for s in range(T):
        if mutate != "map_early" or s == 0:
            move(s)
        if staged:
            w.acc("STAGE_NEXT", "STAGE", min(s + 1, T - 1), -1, "R")
        if s > 0:
            w.acc("EDGE_PREV", "EDGE", (s - 1) & 1, s - 1, "W")
        w.acc("INFO_W", "INFO", 0 if mutate == "single_info_slot" else s & 1, s, "W")
        if s == T - 1:
            w.acc("EDGE_LAST", "EDGE", last_edge, s, "W")
        if mutate == "map_early" and s + 1 < T:
            move(s + 1)
        w.barrier()                                        # barrier s + 1
    w.barrier()                                            # barrier T + 1

    # ---- the two store waves ----
    for par in (0, 1):
        w = _Wave(1 + par, out)
        prologue(w)
        w.acc("RTAB_W", "RTAB", par, -1, "W")

        def fold(q0, cnt):
            for r in range(cnt):
                w.acc("FOLD", "CODE", (q0 + r) % ring, q0 + r, "R")
            for half in (0, 1):
                w.acc("FOLD", "RTAB", half, -1, "R")

        def part_a(q):
            w.acc("INFO_R", "INFO", 0 if mutate == "single_info_slot" else q & 1, q, "R")
            w.acc("MAP_R", "MAP", q & 1, q, "R")
            w.acc("IMG_W", "IMG", par, q, "W")

        def part_b(q):
            w.acc("IMG_R", "IMG", par, q, "R")
            w.acc("EDGE_R", "EDGE", last_edge if q + 1 == T else q & 1, q, "R")
            w.acc("CODE_W", "CODE", q % ring, q, "W")
            if q % 16 == 15 and q + 1 != T:
                fold(q - 15, 16)

        for s in range(1, T + 1):
            w.barrier()                                    # barrier s
            q = s - 1
            if q & 1 == par:
                part_a(q)
                if q == T - 1:
                    part_b(q)
                    if mutate == "early_last_fold":
                        fold((T - 1) & ~15, ((T - 1) & 15) + 1)
            elif q >= 1:
                part_b(q - 1)
        w.barrier()                                        # barrier T + 1
        if (T - 1) & 1 == par and mutate != "early_last_fold":
            fold((T - 1) & ~15, ((T - 1) & 15) + 1)
    return out


def _is_write(r):
    return r.kind != "R"


def check(records, nbarriers=None, T=None):
    """The findings of three rules, [] when the records are in order:
    conflict   two accesses to one (resource, slot) by different waves in one interval, at
               least one of them a write or RMW (two SHARE writes do not conflict);
    stale / no write
               a tagged read must see a write of its tag: among the writes to its slot that
               are ordered before it -- in an earlier interval, or earlier in the same
               wave's program order -- the latest must carry the read's tag;
    barriers   every wave passed T + 2 barriers (when nbarriers and T are given)."""
    findings = []
    by_slot = collections.defaultdict(list)
    for r in records:
        by_slot[(r.res, r.slot)].append(r)
    for (res, slot), rs in sorted(by_slot.items()):
        by_int = collections.defaultdict(list)
        for r in rs:
            by_int[r.interval].append(r)
        for interval, group in sorted(by_int.items()):
            seen = set()
            for i, x in enumerate(group):
                for y in group[i + 1:]:
                    if x.wave == y.wave or not (_is_write(x) or _is_write(y)):
                        continue
                    if x.kind == "SHARE" and y.kind == "SHARE":
                        continue
                    waves = tuple(sorted((x.wave, y.wave)))
                    if waves in seen:
                        continue
                    seen.add(waves)
                    findings.append(Finding("conflict", res, slot, interval, waves,
                                            "%s %s(tag %d) / %s %s(tag %d)" % (x.site, x.kind, x.tag,
                                                                               y.site, y.kind, y.tag)))
        writes = [r for r in rs if _is_write(r)]
        for r in rs:
            if r.kind != "R" or r.tag < 0:
                continue
            before = [x for x in writes
                      if x.interval < r.interval or (x.wave == r.wave and x.seq < r.seq)]
            latest = max(before, key=lambda x: (x.interval, x.seq)) if before else None
            if latest is not None and latest.tag == r.tag:
                continue
            rule = "stale" if any(x.tag == r.tag for x in before) else "no write"
            findings.append(Finding(rule, res, slot, r.interval, (r.wave,),
                                    "%s reads tag %d, latest write before it: %s"
                                    % (r.site, r.tag, "none" if latest is None else
                                       "%s tag %d in interval %d" % (latest.site, latest.tag, latest.interval))))
    if nbarriers is not None and T is not None:
        for wave, n in enumerate(nbarriers):
            if n != T + 2:
                findings.append(Finding("barriers", None, None, None, (wave,),
                                        "%d barriers, expected %d" % (n, T + 2)))
    return findings


def compare(records, expected):
    """Differences between logged records and expected ones, [] when they agree: per wave and
    interval the two multisets of (site, resource, slot, tag, kind) are equal, and a wave
    that writes and reads its IMG slot in one interval does so in program order."""
    def bags(recs):
        b = collections.defaultdict(collections.Counter)
        for r in recs:
            b[(r.wave, r.interval)][r[3:]] += 1
        return b
    got, exp = bags(records), bags(expected)
    diffs = []
    for key in sorted(set(got) | set(exp)):
        if got.get(key) != exp.get(key):
            g, e = got.get(key, collections.Counter()), exp.get(key, collections.Counter())
            diffs.append("wave %d interval %d: unexpected %s, missing %s"
                         % (key + (sorted((g - e).elements()), sorted((e - g).elements()))))
    for r in records:
        if r.res == "IMG" and r.kind == "R":
            if not any(x.res == "IMG" and x.kind == "W" and x.wave == r.wave and x.tag == r.tag and
                       (x.interval < r.interval or (x.interval == r.interval and x.seq < r.seq))
                       for x in records):
                diffs.append("wave %d: IMG read of tag %d (interval %d) not after its write"
                             % (r.wave, r.tag, r.interval))
    return diffs


def decode(n, rec):
    """Records from a mapfx_split_probe_trace: n[3] counts, rec[3][PROBE_CAP][2] words."""
    out = []
    for wave in range(3):
        for i in range(int(n[wave])):
            w0, w1 = int(rec[wave][i][0]), int(rec[wave][i][1])
            out.append(Rec(wave, w0 & 0xFFFF, (w0 >> 16) - 1, SITES[w1 & 0xFF],
                           RESOURCES[(w1 >> 8) & 0xF], (w1 >> 16) & 0xFF, ((w1 >> 24) & 0xFF) - 1,
                           KINDS[(w1 >> 12) & 0xF]))
    return out
