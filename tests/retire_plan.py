"""Plans for the retirement recall tests (CPU only; imports no GPU code).

Between the launches of one crack run the library retires what is cracked: scan_mark_cracked per line, then
scan_mg_rebuild rebuilds the active ESSID groups, their spread over the multi-group PBKDF2 launches, the per-class line
lists and every line's PMK offset (its group's index inside its launch x batch).  A mistake there fails silently: a
genuine crack is not reported.  A plan here is a hash file for a generator whose candidate index fixes the batch (a
mask, or a chain of two lists), with every line's PSK placed at an index inside a CHOSEN batch, so that the run walks
through chosen retirement patterns; and a model of scan_create / scan_mg_rebuild that says, per batch, which groups are
still active and which lines are still verified.  With one worker on one device the library's scan-work counters
(dwpa_debug_scan_work) must equal the model exactly: the scanner thread retires, scans, reads hits and reports in
sequence, so what batch b cracks is retired before batch b + 1 launches.

  plan(name) -> {"name", "lines" (file order), "psk" / "pmk" / "index" / "batch" / "essid" / "cls" / "never" per line
                 (psk None: can never match; index, batch None: never cracks), "records", "record_batch" {record:
                 batch}, "crackable", "batch_size", "nbatches", "keyspace", "groups" (sorted ESSIDs), "table" (file
                 indices in the scan's line order), per batch run "active_groups", "active" = |active_b|, "uncracked"
                 = |uncracked_b|, "launch_sizes" and "launches" = their number, "work" {groups_derived,
                 pbkdf2_launches, line_rows}, and the generator: "mask" + "custom", or "chain" [list A, list B] +
                 "kept_per_batch"}
"""
import functools
import os
import random
from concurrent.futures import ThreadPoolExecutor

from oracle import oracle as O
from tests import test_gpu_recall as R

NC = R.NC
THREADS = min(16, os.cpu_count() or 8)
STRIDE = 16  # every STRIDE-th line also gets the oracle's whole check, derive included
MG_SLOTS = 1 << 24  # engine.cpp: candidate slots per multi-group PBKDF2 launch
CLASSES = (0, 1, 2, 3)  # verify classes in the scan's order: PMKID, keyver 1, 2, 3

A_MASK, A_CUSTOM, A_BATCH, A_K = b"?1" * 10, (b"01",), 64, 1024
B_BATCH, B_NA, B_NB = 1 << 20, 4096, 2048
B_LONG = {0: b"retire", 1000: b"REcall", 2047: b"b-2047"}  # the 6-byte words of list B: the only kept continuations
B_ACTIVE = (40, 33, 32, 17, 16, 15, 1, 1)
B_LAUNCHES = (3, 3, 2, 2, 1, 1, 1, 1)


# ---------------------------------------------------------------------------------------------------------------
# the model of scan_create and scan_mg_rebuild
# ---------------------------------------------------------------------------------------------------------------
def table_order(essid, cls):
    """File indices in the scan's line order: groups by ESSID bytes (std::map<std::string>), inside a group by verify
    class with a stable sort (file order within a class).  Lines are those the scan accepts, `never` ones included."""
    out = []
    for e in sorted(set(essid)):
        idx = [i for i in range(len(essid)) if essid[i] == e]
        out += sorted(idx, key=lambda i: cls[i])  # sorted() is stable, as std::stable_sort
    return out


def spread(nact, per):
    """Sizes of the PBKDF2 launches of `nact` active groups: ceil(nact / per) launches whose sizes differ by at most
    one, the larger ones first."""
    launches = -(-nact // per)
    return [nact // launches + (1 if c < nact % launches else 0) for c in range(launches)]


def simulate(essid, batch, never, batch_size, nbatches):
    """One worker's run: per batch run, the active groups (sorted) and the number of uncracked lines before it.  The
    run ends after the batch that cracks the last crackable line, or with the keyspace."""
    per = max(1, MG_SLOTS // batch_size)
    groups = sorted(set(essid))
    live = [i for i in range(len(essid)) if not never[i]]
    active, uncracked, launches = [], [], []
    for b in range(nbatches):
        left = [i for i in live if batch[i] is None or batch[i] >= b]
        if not left:
            break
        act = [g for g in groups if any(essid[i] == g for i in left)]
        active.append(act)
        uncracked.append(len(left))
        launches.append(spread(len(act), per))
    work = {"groups_derived": sum(len(a) for a in active), "pbkdf2_launches": sum(len(s) for s in launches),
            "line_rows": sum(uncracked)}
    return active, uncracked, launches, work


# ---------------------------------------------------------------------------------------------------------------
# building a plan
# ---------------------------------------------------------------------------------------------------------------
def _short_target(line):
    """The line with its PMKID / MIC cut to 8 bytes: strncmp over 16 bytes never matches (common.php:186,280)."""
    f = line.split(b"*")
    f[2] = f[2][:16]
    return b"*".join(f)


class _Slot:
    """One line to be: its group, verify class, and -- set later -- scheduled batch, PSK and candidate index."""

    def __init__(self, essid, cls, never=False):
        self.essid, self.cls, self.never = essid, cls, never
        self.batch = self.psk = self.index = None


def _finish(name, slots, rng, batch_size, nbatches, extra):
    """slots in file order with batch / psk set.  Builds the lines (each from its PMK, as test_gpu_recall._line),
    asserts every one against the C oracle, and runs the model."""
    by_essid = {}
    for s in slots:
        by_essid.setdefault(s.essid, []).append(s)
    for essid, ss in by_essid.items():  # one PBKDF2 call per group
        raw = O.c_pbkdf2_many([s.psk for s in ss], essid, threads=THREADS)
        for k, s in enumerate(ss):
            s.pmk = raw[32 * k:32 * k + 32]
    lines, want = [], []
    for k, s in enumerate(slots):
        off, endian = R.OFFSETS[k // 4 % 8], ("LE", "BE")[k // 32 % 2]
        line = R._line(s.cls, off, endian, s.psk, s.essid, s.pmk, rng)
        if s.never:
            line = _short_target(line)
        lines.append(line)
        want.append((None, None) if s.cls == 0 else (off, endian))
    assert len(set(lines)) == len(lines)

    def alone(k):  # the PSK and its PMK handed over: no derive
        return O.c_check_key_m22000(lines[k], [slots[k].psk], slots[k].pmk, NC)

    with ThreadPoolExecutor(THREADS) as ex:
        one = list(ex.map(alone, range(len(slots))))
        sel = range(0, len(slots), STRIDE)
        whole = dict(zip(sel, ex.map(lambda k: O.c_check_key_m22000(lines[k], [slots[k].psk], False, NC), sel)))
    for k, s in enumerate(slots):
        if s.never:
            assert one[k] is False, (name, k, one[k])
        else:  # the PSK and the planted correction (offset 0 has no endian)
            off, endian = want[k]
            assert one[k] and one[k][0] == s.psk and one[k][3] == s.pmk and one[k][1] == off and \
                (not off or one[k][2] == endian), (name, k, one[k][:3] if one[k] else one[k])
        if k in whole:
            assert whole[k] == one[k], (name, k, "whole oracle call")
    seen = {(s.cls, w) for s, w in zip(slots, want) if s.cls and not s.never}
    for kv in (1, 2, 3):  # every keyver carries both endians and an offset of both signs
        assert {en for c, (o, en) in seen if c == kv and o} == {"LE", "BE"}, (name, kv)
        assert {o > 0 for c, (o, en) in seen if c == kv and o} == {False, True}, (name, kv)

    essid, cls = [s.essid for s in slots], [s.cls for s in slots]
    batch, never = [s.batch for s in slots], [s.never for s in slots]
    crack = [k for k, s in enumerate(slots) if not s.never and s.batch is not None]
    records = R._records([lines[k] for k in crack], [slots[k].psk for k in crack])
    assert len(set(records)) == len(records)
    active, uncracked, launches, work = simulate(essid, batch, never, batch_size, nbatches)
    p = {"name": name, "lines": lines, "psk": [None if s.never else s.psk for s in slots],
         "pmk": [s.pmk for s in slots],
         "index": [s.index for s in slots], "batch": batch, "essid": essid, "cls": cls, "never": never,
         "records": records, "record_batch": {r: batch[k] for r, k in zip(records, crack)}, "crackable": len(crack),
         "batch_size": batch_size, "nbatches": len(active), "groups": sorted(set(essid)),
         "table": table_order(essid, cls), "active_groups": active, "active": [len(a) for a in active],
         "uncracked": uncracked, "launches": [len(s) for s in launches], "launch_sizes": launches, "work": work}
    p.update(extra)
    return p


def _indices(slots, index_of):
    """A distinct candidate of its scheduled batch for every line that cracks: s.index, s.psk."""
    by_batch = {}
    for s in slots:
        if not s.never and s.batch is not None:
            by_batch.setdefault(s.batch, []).append(s)
    for b, ss in by_batch.items():
        for s, j in zip(ss, index_of(b, len(ss))):
            s.index, s.psk = j


# --- plan A ---------------------------------------------------------------------------------------------------
A_ESSIDS = {"first": b"!retire-first",               # 0x21 sorts before every letter
            "until_end": b"retire-1-until-the-end",
            "front_to_back": b"retire-2-front-to-back",
            "single": b"retire-3-single",
            "inside_out": b"retire-4-inside-out-" + bytes(0x61 + i % 26 for i in range(32)),  # 52: 2 salt blocks
            "class_at_once": b"retire-5-a-class-at-once",
            "back_to_front": b"retire-6-back-to-front",
            "never_finishes": b"retire-7-never-finishes"}
A_OUTSIDE = b"0101010121"  # '2' is not in ?1


def a_candidate(i):
    return b"%010d" % int(bin(i)[2:])


def _plan_a():
    rng = random.Random(0xA7E71)
    assert len(A_ESSIDS["inside_out"]) == 52 and sorted(A_ESSIDS.values()) == list(A_ESSIDS.values())
    slots = []
    for pat, essid in A_ESSIDS.items():
        if pat == "single":
            slots.append(_Slot(essid, 3))
            continue
        slots += [_Slot(essid, c) for c in CLASSES for _ in range(3)]  # runs of 3 lines per class
    nf = A_ESSIDS["never_finishes"]
    outside = _Slot(nf, 2)
    slots += [outside, _Slot(nf, 0, never=True), _Slot(nf, 1, never=True)]
    rng.shuffle(slots)  # the hash file's order: line_of / input_of are not the identity
    essid, cls = [s.essid for s in slots], [s.cls for s in slots]
    table = table_order(essid, cls)
    assert table != sorted(table)
    for pat, e in A_ESSIDS.items():  # t: position inside the group in the scan's line order
        grp = [slots[i] for i in table if slots[i].essid == e and not slots[i].never and slots[i] is not outside]
        for t, s in enumerate(grp):
            run, at = divmod(t, 3)
            assert pat == "single" or s.cls == run
            s.batch = {"first": 0,
                       "until_end": 15,
                       "front_to_back": 1 + t,                       # batches 1..12
                       "single": 7,
                       "inside_out": 2 + 3 * run + (1, 0, 2)[at],    # middle, first, last of every run
                       "class_at_once": {2: 3, 0: 6, 1: 9, 3: 14}[s.cls],
                       "back_to_front": 12 - t,                      # batches 12..1
                       "never_finishes": (0, 5, 10, 15)[run]}[pat]
    per_batch = A_K // A_BATCH
    assert per_batch == 16

    def index_of(b, n):
        assert n <= A_BATCH
        return [(A_BATCH * b + j, a_candidate(A_BATCH * b + j)) for j in rng.sample(range(A_BATCH), n)]

    _indices(slots, index_of)
    outside.psk = A_OUTSIDE
    for s in slots:
        if s.never:
            s.psk = b"never-" + bytes([0x30 + s.cls]) * 4
    p = _finish("A", slots, rng, A_BATCH, per_batch, {"mask": A_MASK, "custom": A_CUSTOM, "keyspace": A_K})
    assert p["nbatches"] == 16 and p["crackable"] == 6 * 12 + 1 + 12 and len(p["lines"]) == p["crackable"] + 3
    return p


# --- plan B ---------------------------------------------------------------------------------------------------
def b_lists():
    a = [b"%03x" % i for i in range(B_NA)]
    b = [B_LONG.get(i, b"%03x" % i) for i in range(B_NB)]
    return a, b


def _between_survivors(act, sizes, leaving):
    """A leaving group with a survivor before and after it inside one launch."""
    at = 0
    for n in sizes:
        chunk = act[at:at + n]
        at += n
        stay = [k for k, g in enumerate(chunk) if g not in leaving]
        if stay and any(stay[0] < k < stay[-1] for k, g in enumerate(chunk) if g in leaving):
            return True
    return False


def _plan_b():
    rng = random.Random(0xB7E71)
    n = B_ACTIVE[0]
    essids = [b"retire-b-%02d" % g for g in range(n)]
    essids[20] += bytes(0x41 + i % 26 for i in range(52 - len(essids[20])))  # 52 bytes, still sorted between 19 and 21
    assert sorted(essids) == essids and len(essids[20]) == 52
    order = list(range(n))
    rng.shuffle(order)  # which groups leave at each step
    last, at = {}, 0
    for b in range(len(B_ACTIVE) - 1):
        for g in order[at:at + B_ACTIVE[b] - B_ACTIVE[b + 1]]:
            last[g] = b  # the last batch in which group g cracks a line
        at += B_ACTIVE[b] - B_ACTIVE[b + 1]
    stays = order[at:]
    assert len(stays) == 1 and len(last) == n - 1
    slots, kinds = [], 0
    for g in range(n):
        if g == stays[0]:  # cracks in batches 6 and 7 and keeps one line no candidate opens
            sched = [6, 7, None]
        else:  # 2-3 lines: one in the group's last batch, the others in it or earlier
            sched = [last[g]] + [rng.randint(0, last[g]) for _ in range(1 + g % 2)]
        for b in sched:
            s = _Slot(essids[g], kinds % 4)
            s.batch = b
            kinds += 1
            slots.append(s)
    rng.shuffle(slots)
    la, lb = b_lists()
    rows = B_BATCH // B_NB  # A-words per batch
    assert rows == 512 and B_NA // rows == len(B_ACTIVE)

    def index_of(b, k):
        pairs = rng.sample([(a, j) for a in range(rows * b, rows * b + rows) for j in sorted(B_LONG)], k)
        return [(a * B_NB + j, la[a] + lb[j]) for a, j in pairs]

    _indices(slots, index_of)
    for s in slots:
        if s.batch is None:
            s.psk = b"000retirE"  # 'retirE' is no word of list B
    p = _finish("B", slots, rng, B_BATCH, len(B_ACTIVE), {"chain": [la, lb], "keyspace": B_NA * B_NB,
                                                          "kept_per_batch": rows * len(B_LONG)})
    assert tuple(p["active"]) == B_ACTIVE and tuple(p["launches"]) == B_LAUNCHES
    assert {len(g) for g in (([s for s in slots if s.essid == e]) for e in essids)} == {2, 3}
    steps = [(p["active_groups"][b], p["launch_sizes"][b], set(p["active_groups"][b]) - set(p["active_groups"][b + 1]))
             for b in range(p["nbatches"] - 1)]
    assert any(act[0] in gone for act, _, gone in steps), "the sorted-first active group never leaves"
    assert any(act[-1] in gone for act, _, gone in steps), "the sorted-last active group never leaves"
    assert any(_between_survivors(*st) for st in steps), "no group leaves from between two survivors of a launch"
    for b in range(1, p["nbatches"]):  # every survivor of a step has a line that cracks in a later batch
        for g in p["active_groups"][b]:
            assert any(s.batch is not None and s.batch >= b for s in slots if s.essid == g), (b, g)
    return p


@functools.lru_cache(maxsize=None)
def plan(name):
    if name == "A":
        return _plan_a()
    if name == "B":
        return _plan_b()
    raise KeyError(name)
