"""One seeded random walk over the whole surface of a long-lived index -- TEST INFRASTRUCTURE, not product code.  tests/RANDOM_WALK.md
is the page about it.

``run(target, model, rng, steps, on_event)`` draws one mutation per step, applies it to ``target`` (anything with FlatIndex's surface:
the GPU index, or another model) and to ``model`` (tests/index_model.py), checks the sizes and every filter and grouping, and then
makes a random subset of the twelve search forms on both, comparing every output exactly (floats by their bits).  The draw depends
on the model's state alone, so one seed gives one sequence whatever the target is -- until the target differs, and then the walk stops.

The weights of the draw lean towards what the walk exists for (``EVENTS``): an operation that brings a missing event closer is
preferred, the rest stays random.  tests/test_random_walk_model.py asserts on the CPU that every seed reaches every event.
"""
import numpy as np

from conftest import bits
from index_model import Capacities
from memex_amd._lib import MemexHipError

STEPS = 40
MAX_ROWS = 7800
GROWTHS = (1024, 1536, 2304)           # the capacities ensure_capacity (memex_amd/csrc/index.hip) steps through from an empty index:
                                       # PER SHARD, so a handle of G shards outgrows the last of them at about G x 2304 rows
MIN_BLOCK = 64                         # the list blocks (ensure_mmr_lists, ensure_byid_lists, ...) never hold fewer entries per query
OFFSETS = (0, 1000, 2 ** 40)
ADD_SIZES = (1, 31, 64, 65, 200, 1000, 1500)

# the layouts of tests/test_feature_random_ops_gpu.py; the CPU test walks the same seeds
CASES = [
    dict(name="int8-d384", seed=101, d=384, copy="i8", cone=False, compressed=False, devices=None, block_rows=0),
    dict(name="bf16-cone-d200", seed=202, d=200, copy="bf16", cone=True, compressed=False, devices=None, block_rows=0),
    dict(name="nocopy-d100", seed=303, d=100, copy="none", cone=False, compressed=False, devices=None, block_rows=0),
    dict(name="compressed-d72", seed=404, d=72, copy=None, cone=False, compressed=True, devices=None, block_rows=0),
    dict(name="3shards-d100", seed=505, d=100, copy=None, cone=False, compressed=False, devices=[0, 0, 0], block_rows=96),
    dict(name="2shards-compressed-d72", seed=606, d=72, copy=None, cone=False, compressed=True, devices=[0, 0], block_rows=64),
]

EVENTS = (
    "grow_1024", "grow_1536", "grow_2304",          # EVERY shard's rows outgrow storage of this capacity under one live filter and
                                                    # grouping, both searched after
    "fetch_up", "fetch_down_other_form",            # the shared candidate lists: a larger fetch than ever (and than the block's first
                                                    # 64 entries per query: it is allocated anew), then another form with a smaller one
    "by_id_wider", "like_wider", "score_ids_wider",  # a larger list width than any call of the form before, and than 64
    "auto_exact_auto",                              # one form on AUTO, on the EXACT path, on AUTO again
    "add_after_compact", "by_id_after_compact", "like_after_compact", "score_ids_after_compact",
    "offset_edit_search",                           # set_id_offset under live handles, then an edit of each by id and a search with them
    "stale_filter_compact", "stale_grouping_compact", "stale_filter_load", "stale_grouping_load", "stale_filter_clear",
    "stale_grouping_clear",                         # made stale by each cause, used (it raised), replaced
    "copy_switch_between_forms",
    "complete_by_short_list",                       # a grouped search finds fewer than k groups in a list of k or more, but fewer than fetch, rows
    "removed_row_everywhere",                       # a removed row that was in a filter and keyed: by-id query, like example, score_ids candidate
)

SHARED = ("mmr", "fused", "grouped", "grouped_f")
FORMS = ("search", "filtered", "with", "range", "by_id", "range_by_id", "like", "score_ids") + SHARED

F32, F64, INT = "f32", "f64", "int"
LISTS = (("ids", INT), ("scores", F32), ("dists", F32), ("n_found", INT))
FIELDS = {
    "search": LISTS, "filtered": LISTS, "with": LISTS, "mmr": LISTS, "by_id": LISTS,
    "range": LISTS + (("n_in_range", INT),), "range_by_id": LISTS + (("n_in_range", INT),),
    "fused": LISTS + (("best_sub", INT), ("fused", F64)),
    "grouped": (("ids", INT), ("scores", F32), ("dists", F32), ("keys", INT), ("group_rows", INT), ("n_found", INT), ("complete", INT)),
    "like": LISTS + (("n_used", INT), ("combined", F32)),
    "score_ids": (("scores", F32), ("dists", F32), ("order", INT), ("n_found", INT)),
}
FIELDS["grouped_f"] = FIELDS["grouped"]


class Pair:
    """one filter or grouping: the target's handle and the model's"""

    def __init__(self, kind, t, m):
        self.kind, self.t, self.m = kind, t, m
        self.cause = None               # what made it stale
        self.raised = False             # it was used while stale, and raised


class Walk:
    def __init__(self, target, model, rng, on_event=None, store_dir="store", cone=False, tag="walk", shards=1, block_rows=0):
        self.target, self.model, self.rng = target, model, rng
        self.capacity = Capacities(shards, block_rows)                     # what the storage of every shard of the target holds
        self.on_event = on_event or (lambda name: None)
        self.store_dir, self.tag = str(store_dir), tag
        self.d = model.dim
        self.axis = rng.standard_normal(self.d) * 4.0 if cone else None
        self.pairs = []
        self.seen = set()
        self.what = f"{tag}: start"
        self.step_no = 0
        self.exact_step = False
        self.copy_pending = None
        self.forced = []                # forms the next steps must make (an event waits for them)
        # event book-keeping
        self.crossing = {}              # capacity -> [shards that outgrew it, pairs alive at every one of those appends]
        self.grown = {}                 # capacity every shard outgrew -> [pairs alive at the crossings, forms still owed]
        self.max_fetch, self.max_fetch_form = None, None
        self.widest = {}
        self.path = {}                  # form -> 0 nothing, 1 AUTO, 2 AUTO then EXACT
        self.compacted = False          # a compaction dropped rows, and no append, load or clear came since
        self.moved = None               # (a, b): the compaction gave the rows a .. b - 1 new ids (until a load or clear)
        self.offset_owed = None         # after set_id_offset under live handles: what is still owed
        self.marked = set()             # 0-based removed rows that were in a filter and keyed
        self.marked_named = {}
        self.document = None            # the filter of op_document, until a grouped search used it
        self.log = []                   # what every step did, for the message of a failure that needs the history

    # -- events -------------------------------------------------------------------------------------------------------------------
    def event(self, name):
        assert name in EVENTS, name
        if name not in self.seen:
            self.seen.add(name)
        self.on_event(name)

    def missing(self, name):
        return name not in self.seen

    # -- comparing ----------------------------------------------------------------------------------------------------------------
    def fail(self, msg):
        raise AssertionError(f"{self.what}: {msg}")

    def outcome(self, fn):
        try:
            return "ok", fn()
        except MemexHipError as e:
            return "error", e

    def both(self, call, fn, pairs=()):
        """fn(index, *handles) on the model and on the target -> (model's outcome, target's); both raise or neither"""
        want = self.outcome(lambda: fn(self.model, *[p.m for p in pairs]))
        got = self.outcome(lambda: fn(self.target, *[p.t for p in pairs]))
        if want[0] != got[0]:
            self.fail(f"{call}: the model gives {want[0]} ({want[1]!r:.200}), the target {got[0]} ({got[1]!r:.200})")
        if want[0] == "error" and want[1].code != got[1].code:
            self.fail(f"{call}: the model raises code {want[1].code}, the target {got[1].code} ({got[1]})")
        return want, got

    def same(self, call, got, want, fields):
        if len(got) != len(fields) or len(want) != len(fields):
            self.fail(f"{call}: {len(got)} outputs, the model has {len(want)}")
        for g, w, (name, kind) in zip(got, want, fields):
            g, w = np.asarray(g), np.asarray(w)
            if g.shape != w.shape:
                self.fail(f"{call}: {name} has shape {g.shape}, the model's {w.shape}")
            if kind == F32:
                g, w = bits(g), bits(w)
            elif kind == F64:
                g, w = np.ascontiguousarray(g, np.float64).view(np.uint64), np.ascontiguousarray(w, np.float64).view(np.uint64)
            else:
                g, w = g.astype(np.int64) if g.dtype != np.uint64 else g, w.astype(np.int64) if w.dtype != np.uint64 else w
            if not np.array_equal(g, w):
                at = np.argwhere(np.atleast_1d(g != w))[0].tolist()
                self.fail(f"{call}: {name} differs, first at {at}: target {np.atleast_1d(g)[tuple(at)]}, model {np.atleast_1d(w)[tuple(at)]}")

    def must_be_stale(self, call, fn, pairs):
        want, got = self.both(call, fn, pairs)
        if want[0] != "error":
            self.fail(f"{call}: the model does not raise on a stale handle")
        if "stale" not in str(got[1]):
            self.fail(f"{call}: the target's message does not say stale: {got[1]}")

    # -- state helpers ------------------------------------------------------------------------------------------------------------
    def live(self, kind):
        return [p for p in self.pairs if p.kind == kind and p.cause is None]

    def stale(self):
        return [p for p in self.pairs if p.cause is not None]

    def n(self):
        return len(self.model)

    def off(self):
        return self.model.id_offset

    def pick_pair(self, kind):
        """a live handle of the kind: one an event still waits for, else any"""
        live = self.live(kind)
        if kind == "filter" and self.document in live:
            return self.document
        owed = [p for p in live if self.owed(p)]
        return owed[0] if owed else self.pick_of(live)

    def rows_in_all(self):
        """live rows that are in a live filter and keyed in a live grouping"""
        f, g = self.live("filter"), self.live("grouping")
        if not f or not g or not self.n():
            return np.zeros(0, np.int64)
        in_f = np.logical_or.reduce([p.m.mask() for p in f])
        keyed = np.logical_or.reduce([p.m.row_keys() != 0 for p in g])
        return np.flatnonzero(in_f & keyed & self.model.alive)

    def make_rows(self, m):
        rng = self.rng
        Y = rng.standard_normal((m, self.d))
        if self.axis is not None:
            Y = Y + self.axis
        Y = (Y * rng.uniform(0.5, 3.0, (m, 1))).astype(np.float32)
        if rng.random() < 0.35:
            Y[int(rng.integers(0, m))] = 0.0                               # a zero row
        if m >= 4 and rng.random() < 0.35:
            a = int(rng.integers(0, m - 2))
            Y[a:a + int(rng.integers(2, min(m - a, 40) + 1))] = Y[a]       # a run of exact duplicates
        return Y

    def queries(self, B):
        rng = self.rng
        Q = rng.standard_normal((B, self.d))
        if self.axis is not None:
            Q[::2] += self.axis
        Q = Q.astype(np.float32)
        if self.n():
            Q[int(rng.integers(0, B))] = self.model.rows[int(rng.integers(0, self.n()))] * np.float32(2.0)   # a stored row x 2
        if rng.random() < 0.25:
            Q[int(rng.integers(0, B))] = 0.0
        return Q

    def some_ids(self, m, strange=True):
        """m ids: mostly rows of the index, and with `strange` a removed row and ids that name no row among them"""
        rng, n, off = self.rng, self.n(), self.off()
        ids = (rng.integers(0, max(n, 1), m) + 1 + off).astype(np.uint64)
        if strange:
            dead = np.flatnonzero(~self.model.alive)
            pool = [off + n + 1, 0, off + n + 1 + int(rng.integers(1, 500)), off if off else 2 ** 41]
            marked = sorted(self.marked)
            for j in rng.permutation(m)[:max(1, m // 3)].tolist():
                r = rng.random()
                if dead.size and r < 0.5:
                    ids[j] = int(marked[int(rng.integers(0, len(marked)))] if marked and r < 0.3 else dead[int(rng.integers(0, dead.size))]) + 1 + off
                else:
                    ids[j] = pool[int(rng.integers(0, len(pool)))]
        return ids

    def random_ranges(self, m):
        rng, n, off = self.rng, self.n(), self.off()
        lo = rng.integers(max(off - 20, 0), off + n + 40, m)
        ln = rng.integers(0, max(n // 3, 2), m)
        if rng.random() < 0.4:                                             # narrow ranges: a filter of a few dozen rows
            ln = rng.integers(0, 40, m)
        return np.stack([lo, lo + ln], axis=1).astype(np.uint64)

    def note_named(self, form, ids):
        """a by-id / like / score_ids call named these ids: events about ids that moved and about removed rows"""
        rows = np.asarray(ids, dtype=np.uint64).reshape(-1).astype(object) - self.off() - 1
        rows = [int(r) for r in rows if 0 <= r < self.n()]
        if self.moved and any(self.moved[0] <= r < self.moved[1] and self.model.alive[r] for r in rows):
            self.event(f"{form}_after_compact")
        hit = self.marked.intersection(rows)
        for r in hit:
            self.marked_named.setdefault(r, set()).add(form)
            if len(self.marked_named[r]) == 3:
                self.event("removed_row_everywhere")

    def pick_width(self, form, widths, extra=0):
        """a value whose width (value + extra) the form has not reached yet while its event is missing: the smallest first"""
        if form not in self.widest:
            return min(widths)
        wider = [v for v in widths if v + extra > max(self.widest[form], MIN_BLOCK)]
        return min(wider) if wider and self.missing(f"{form}_wider") else self.pick_of(widths)

    def pick_fetch(self, form, k, fetches):
        """a fetch that serves the events of the shared lists while they are missing, else any"""
        base = "grouped" if form == "grouped_f" else form
        fetches = sorted({max(k, f) for f in fetches})
        if self.max_fetch is None:
            return fetches[0]
        if self.missing("fetch_up"):
            up = [f for f in fetches if f > max(self.max_fetch, MIN_BLOCK)]
            return up[0] if up else self.pick_of(fetches)
        if self.missing("fetch_down_other_form") and base != self.max_fetch_form:
            down = [f for f in fetches if f < self.max_fetch]
            return down[-1] if down else self.pick_of(fetches)
        return self.pick_of(fetches)

    def name_marked(self, ids, at):
        """while the event waits for it: the removed row that was in a filter and keyed, in slot `at`"""
        if self.marked and self.missing("removed_row_everywhere"):
            ids[at] = min(self.marked) + 1 + self.off()

    def name_moved(self, form, ids, at):
        """while the event waits for it: a live row that the last compaction moved, in slot `at`"""
        if self.moved and self.missing(f"{form}_after_compact"):
            moved = np.flatnonzero(self.model.alive[self.moved[0]:self.moved[1]]) + self.moved[0]
            if moved.size:
                ids[at] = int(moved[int(self.rng.integers(0, moved.size))]) + 1 + self.off()

    def query_ids(self, form, B):
        """B ids of stored rows for a by-id form.  As far as B has room: the row an event waits for (the marked one, a moved one),
        a removed row and an id that names no row, each in a slot of its own; the rest as some_ids draws them"""
        rng, n, off = self.rng, self.n(), self.off()
        ids = self.some_ids(B)
        dead = np.flatnonzero(~self.model.alive)
        special = [lambda at: self.name_marked(ids, at), lambda at: self.name_moved(form, ids, at)]
        rest = [lambda at: ids.__setitem__(at, self.pick_of((off + n + 1, 0, off + n + 1 + int(rng.integers(1, 500)))))]
        if dead.size:
            rest.append(lambda at: ids.__setitem__(at, int(dead[int(rng.integers(0, dead.size))]) + 1 + off))
        special += [rest[i] for i in rng.permutation(len(rest))]
        for at, put in zip(rng.permutation(B).tolist(), special):
            put(at)
        return ids

    def note_width(self, form, width):
        if form in self.widest and width > max(self.widest[form], MIN_BLOCK):
            self.event(f"{form}_wider")
        self.widest[form] = max(width, self.widest.get(form, 0))

    def note_path(self, form, width):
        exact = self.model.mode == 1 or width > 256
        s = self.path.get(form, 0)
        if s == 0 and not exact:
            s = 1
        elif s == 1 and exact:
            s = 2
        elif s == 2 and not exact:
            s = 3
            self.event("auto_exact_auto")
        self.path[form] = s

    def note_fetch(self, form, fetch):
        base = "grouped" if form == "grouped_f" else form
        if self.max_fetch is not None and fetch > max(self.max_fetch, MIN_BLOCK):
            self.event("fetch_up")
        if "fetch_up" in self.seen and self.max_fetch is not None and fetch < self.max_fetch and base != self.max_fetch_form:
            self.event("fetch_down_other_form")
        if self.max_fetch is None or fetch > self.max_fetch:
            self.max_fetch, self.max_fetch_form = fetch, base

    def note_handles_searched(self, form, pairs):
        for cap, (alive_then, owed) in list(self.grown.items()):
            if all(p in alive_then and p.cause is None for p in pairs):
                owed.discard(form)
                if not owed:
                    del self.grown[cap]
                    self.event(f"grow_{cap}")
        if self.offset_owed and all(p in self.offset_owed["pairs"] and p.cause is None for p in pairs):
            self.offset_owed["owed"].discard(form)
            self.offset_done()

    def offset_done(self):
        if self.offset_owed and not self.offset_owed["owed"]:
            self.offset_owed = None
            self.event("offset_edit_search")

    # -- the draw -----------------------------------------------------------------------------------------------------------------
    def wanted(self):
        """the operations that bring a missing event closer in this state"""
        n, miss = self.n(), self.missing
        if any(p.raised for p in self.stale()):
            return ["handles"]
        if n < 500 and any(miss(e) for e in EVENTS if not e.endswith("_clear")):
            return ["add"]                                                 # rows first: nothing else means much on a handful of them
        if n == 0:
            return ["add"]
        if not self.live("filter") or not self.live("grouping") or not self.rows_in_all().size:
            return ["handles"] if not self.stale() else []
        if self.compacted and miss("add_after_compact"):
            return ["add"]                                                 # before a load or a clear stands between the two
        w = []
        if self.offset_owed:
            w += [op for op in ("fedit", "gedit") if op in self.offset_owed["owed"]]
            return w
        if any(miss(f"grow_{c}") and c not in self.grown for c in GROWTHS) and min(self.capacity.share(n)) <= GROWTHS[-1]:
            w += ["add", "add", "add"]                                     # until the last shard has outgrown the last capacity
        if n >= 600:
            if miss("removed_row_everywhere") and not self.marked:
                w.append("remove")
            if miss("offset_edit_search"):
                w.append("offset")
            if miss("copy_switch_between_forms"):
                w.append("copy")
            if miss("complete_by_short_list"):
                w.append("document")
            if miss("auto_exact_auto") and self.step_no > STEPS // 3:
                w.append("exact")
        grown = not any(miss(f"grow_{c}") for c in GROWTHS)
        if grown or self.step_no > STEPS // 2:
            if miss("stale_filter_compact") or miss("stale_grouping_compact"):
                w.append("compact" if self.model.removed else "remove")
            if miss("stale_filter_load") or miss("stale_grouping_load"):
                w.append("save_load")
            if not self.moved and any(miss(f"{f}_after_compact") for f in ("by_id", "like", "score_ids")):
                w.append("compact" if self.model.removed else "remove")
            if self.step_no >= STEPS - 5 and (miss("stale_filter_clear") or miss("stale_grouping_clear")):
                return ["clear"]                                           # late: the steps before it meet rows, the ones after it few
        return w

    def pick(self):
        rng = self.rng
        w = self.wanted()
        if w and rng.random() < 0.8:
            return w[int(rng.integers(0, len(w)))]
        ops = ["add"] * 4 + ["remove"] * 4 + ["fedit"] * 3 + ["gedit"] * 3 + ["handles"] * 2 + ["offset", "copy", "copy", "exact", "reserve", "document",
                                                                                              "compact", "save_load"]
        if rng.random() < 0.02:
            ops = ["clear"]
        op = ops[int(rng.integers(0, len(ops)))]
        if op == "compact" and any(self.missing(f"grow_{c}") for c in GROWTHS):
            op = "remove"                 # a compaction resets the capacities (Capacities.compacted): after the growths, not among them
        return op

    # -- mutations ----------------------------------------------------------------------------------------------------------------
    def op_add(self):
        rng, n, cap = self.rng, self.n(), self.capacity
        sizes = [s for s in ADD_SIZES if n + s <= MAX_ROWS]
        if not sizes:
            self.what += " (no room: remove)"
            return self.op_remove()

        def waited(s):
            """the shards whose storage an append of s rows moves out of a capacity that an event still waits for"""
            return [(g, old) for g, old, _ in cap.moves(n + s) if old in GROWTHS and self.missing(f"grow_{old}") and old not in self.grown]

        # no shard jumps a capacity in one append: it goes from c to the next of GROWTHS, as ensure_capacity steps when it is outgrown
        sizes = [s for s in sizes if all(new == (max(old + old // 2, 1024) + 63) // 64 * 64 for _, old, new in cap.moves(n + s))] or sizes[:1]
        alive_then = [p for p in self.pairs if p.cause is None and p.m.count()[0] > 0]
        ready = {p.kind for p in alive_then} == {"filter", "grouping"}
        if not ready:                                                      # no crossing before the handles it is about exist
            sizes = [s for s in sizes if not waited(s)]
            if not sizes:
                self.what += " (a filter and a grouping first: handles)"
                return self.op_handles()
        elif any(self.missing(f"grow_{c}") and c not in self.grown for c in GROWTHS):
            sizes = [s for s in sizes if waited(s)] or sizes[-2:]           # across the next capacity, or towards it in large strides
        if n < 500:
            sizes = sizes[-3:]
        m = int(sizes[int(rng.integers(0, len(sizes)))])
        Y = self.make_rows(m)
        self.what += f" {m} rows at {n}"
        first = self.target.add(Y)
        if first != self.model.add(Y):
            self.fail(f"add returned {first}, the model {self.off() + n + 1}")
        stored = self.target.get_rows(n, m)
        if not self.model.compressed and not np.array_equal(bits(stored), bits(Y)):
            self.fail("get_rows does not return the rows that were added")
        self.model.replace_tail(stored)
        if self.compacted:
            self.event("add_after_compact")
            self.compacted = False
        for g, old, new in cap.grow(n + m):
            if old and ready:
                self.what += f", shard {g} moves from {old} to {new} rows"
            if not (ready and old in GROWTHS and self.missing(f"grow_{old}") and old not in self.grown):
                continue
            shards, alive = self.crossing.setdefault(old, [set(), alive_then])
            shards.add(g)
            self.crossing[old][1] = alive = [p for p in alive if p in alive_then]
            if {p.kind for p in alive} != {"filter", "grouping"}:         # the handles of the first shard's crossing are gone
                del self.crossing[old]
            elif len(shards) == cap.shards:                                # the last shard: now the searches
                del self.crossing[old]
                self.grown[old] = [alive, {"with", "grouped_f"}]
                self.forced += ["with", "grouped_f"]

    def op_reserve(self):
        want = self.n() + int(self.rng.choice([0, 100, 700, 2000]))
        if any(old in GROWTHS and self.missing(f"grow_{old}") for _, old, _ in self.capacity.moves(want)):
            want = self.n()               # that capacity is to be outgrown by an append under live handles
        self.what += f" {want}"
        self.capacity.grow(want)
        self.target.reserve(want)
        self.model.reserve(want)

    def op_remove(self):
        rng, n, off = self.rng, self.n(), self.off()
        if n == 0:
            self.what += " (no rows: add)"
            return self.op_add()
        kind = str(rng.choice(["ids", "ids", "run", "tile", "again", "outside"]))
        inside = self.rows_in_all()
        if self.missing("removed_row_everywhere") and not self.marked and inside.size:
            kind = "inside"
        if kind == "inside":
            r = inside[rng.integers(0, inside.size, min(5, inside.size))]
        elif kind == "ids":
            r = rng.integers(0, n, int(rng.integers(1, max(2, min(n // 4, 300)))))
        elif kind == "run":
            a = int(rng.integers(0, n))
            r = np.arange(a, min(n, a + int(rng.integers(1, 200))))
        elif kind == "tile":
            t = int(rng.integers(0, (n + 63) // 64))
            r = np.arange(64 * t, min(n, 64 * t + 64))
        elif kind == "again" and self.model.removed:
            dead = np.flatnonzero(~self.model.alive)
            r = dead[rng.integers(0, dead.size, min(3, dead.size))]
        else:                                                              # an id that names no row: the call fails, nothing is removed
            r = np.r_[rng.integers(0, n, 3), n]
        ids = np.asarray(r, dtype=np.int64).astype(np.uint64) + np.uint64(off + 1)
        self.what += f" {kind}, {len(ids)} ids from {int(ids.min())}"
        inside_set = set(inside.tolist())
        want, got = self.both("remove", lambda idx: idx.remove(ids))
        if want[0] == "ok":
            if want[1] != got[1]:
                self.fail(f"remove counted {got[1]} new removals, the model {want[1]}")
            self.marked.update(int(x) for x in np.asarray(r).tolist() if int(x) in inside_set)
            if self.marked and self.missing("removed_row_everywhere"):
                self.forced += ["by_id", "like", "score_ids"]

    def rows_replaced(self, cause):
        for p in self.pairs:
            if p.cause is None:
                p.cause = cause
        self.grown.clear()
        self.crossing.clear()
        self.offset_owed = None
        self.forced = []
        self.marked.clear()
        self.marked_named.clear()

    def op_compact(self):
        dead = np.flatnonzero(~self.model.alive)
        self.what += f" {dead.size} removed"
        kept = self.target.compact()
        want = self.model.compact()
        if not np.array_equal(kept, want):
            self.fail("compact: kept_ids differ from the model's")
        if dead.size:
            self.rows_replaced("compact")
            self.capacity.compacted(self.n())
            self.compacted = True
            self.moved = (int(dead[0]), self.n()) if dead[0] < self.n() else None      # the rows behind the first one dropped
            if self.moved:
                self.forced += [f for f in ("by_id", "like", "score_ids") if self.missing(f"{f}_after_compact")]

    def op_save_load(self):
        for idx in (self.model, self.target):
            idx.save(self.store_dir)
            idx.load(self.store_dir)
        self.rows_replaced("load")
        self.compacted, self.moved = False, None

    def op_clear(self):
        self.target.clear()
        self.model.clear()
        self.rows_replaced("clear")
        self.compacted, self.moved = False, None

    def op_offset(self):
        others = [o for o in OFFSETS if o != self.off()]
        off = others[int(self.rng.integers(0, len(others)))]
        self.what += f" {off}"
        self.target.set_id_offset(off)
        self.model.set_id_offset(off)
        f, g = self.live("filter"), self.live("grouping")
        if f and g and self.missing("offset_edit_search"):
            self.offset_owed = {"pairs": f + g, "owed": {"fedit", "gedit", "with", "grouped_f"}}
            self.forced += ["with", "grouped_f"]

    def op_copy(self):
        kinds = [k for k in ("i8", "bf16", "none", "auto") if not (k == "none" and self.model.compressed) and k != self.model.copy_kind]
        self.copy_pending = kinds[int(self.rng.integers(0, len(kinds)))]
        self.what += f" {self.copy_pending}, between two checked calls"

    def op_exact(self):
        self.target.set_search_mode(1)
        self.model.set_search_mode(1)
        self.exact_step = True

    def op_fedit(self):
        live = self.live("filter")
        if not live:
            self.what += " (no live filter: handles)"
            return self.op_handles()
        rng = self.rng
        p = self.pick_pair("filter")
        by_ids = bool(rng.random() < 0.5) or bool(self.offset_owed and "fedit" in self.offset_owed["owed"])
        allow = bool(rng.random() < 0.6)
        arg = dict(ids=self.some_ids(int(rng.integers(1, 200)))) if by_ids else dict(ranges=self.random_ranges(int(rng.integers(1, 5))))
        self.what += f" {'allow' if allow else 'deny'} by {'ids' if by_ids else 'ranges'}"
        self.both("filter edit", lambda idx, f: (f.allow if allow else f.deny)(**arg), [p])
        if by_ids and self.offset_owed and p in self.offset_owed["pairs"]:
            self.offset_owed["owed"].discard("fedit")
            self.offset_done()

    def disjoint_ranges(self):
        rng, n, off = self.rng, self.n(), self.off()
        m = int(rng.integers(1, 12))
        cuts = np.sort(rng.integers(0, n + 30, 2 * m)) + off + 1
        r = cuts.reshape(m, 2)
        keys = rng.integers(0, 9, m).astype(np.uint32) * (rng.random(m) > 0.15)
        order = rng.permutation(m)
        return r[order].astype(np.uint64), keys[order].astype(np.uint32)

    def op_gedit(self):
        live = self.live("grouping")
        if not live:
            self.what += " (no live grouping: handles)"
            return self.op_handles()
        rng = self.rng
        p = self.pick_pair("grouping")
        by_ids = bool(rng.random() < 0.5) or bool(self.offset_owed and "gedit" in self.offset_owed["owed"])
        self.what += f" by {'ids' if by_ids else 'ranges'}"
        if by_ids:
            ids = self.some_ids(int(rng.integers(1, 200)))
            keys = (ids % np.uint64(7)).astype(np.uint32) + np.uint32(rng.integers(0, 3))   # one key per id value: repeats agree
            if rng.random() < 0.3:
                keys = np.uint32(rng.integers(0, 5))
            self.both("grouping set_ids", lambda idx, g: g.set_ids(ids, keys), [p])
            if self.offset_owed and p in self.offset_owed["pairs"]:
                self.offset_owed["owed"].discard("gedit")
                self.offset_done()
        else:
            r, keys = self.disjoint_ranges()
            self.both("grouping set_ranges", lambda idx, g: g.set_ranges(r, keys), [p])

    def op_document(self):
        """one document: a short run of rows under one key, and a filter of just that run; a grouped search within it follows"""
        rng, n, off = self.rng, self.n(), self.off()
        if n < 100:
            self.what += " (too few rows: add)"
            return self.op_add()
        if not self.live("grouping"):
            self.what += " (no live grouping: handles)"
            return self.op_handles()
        c = int(rng.integers(20, 60))
        a = int(rng.integers(0, n - c))
        run = np.array([[off + 1 + a, off + 1 + a + c]], dtype=np.uint64)
        key = np.uint32(rng.integers(1, 9))
        self.what += f" rows {a} .. {a + c - 1}, key {key}"
        self.both("grouping set_ranges", lambda idx, g: g.set_ranges(run, key), [self.pick_pair("grouping")])
        free = [p for p in self.live("filter") if not self.owed(p)]
        if len(self.live("filter")) >= 2 and free:
            self.drop_pair(free[0])
        self.document = Pair("filter", self.target.make_filter(ranges=run), self.model.make_filter(ranges=run))
        self.pairs.append(self.document)
        self.forced += ["grouped_f"]

    def new_pair(self, kind):
        rng, n, off = self.rng, self.n(), self.off()
        if kind == "filter":
            if rng.random() < 0.5:
                a = int(rng.integers(0, max(n // 2, 1)))
                arg = dict(ranges=np.array([[off + 1 + a, off + 1 + a + max(n // 2, 1)], [max(off + n - 5, 0), off + n + 50]], dtype=np.uint64))
            else:
                arg = dict(ids=self.some_ids(max(n // 3, 3)))
            p = Pair(kind, self.target.make_filter(**arg), self.model.make_filter(**arg))
        else:
            p = Pair(kind, self.target.make_grouping(), self.model.make_grouping())
            r, keys = self.disjoint_ranges()
            span = np.array([[off + 1, off + n + 1]], dtype=np.uint64)      # every row keyed, then random documents over it
            key = np.uint32(1 + rng.integers(0, 3))
            self.both("grouping set_ranges", lambda idx, g: g.set_ranges(span, key), [p])
            self.both("grouping set_ranges", lambda idx, g: g.set_ranges(r, keys), [p])
        self.pairs.append(p)

    def owed(self, p):
        return (any(p in a for a, _ in self.grown.values()) or any(p in a for _, a in self.crossing.values())
                or bool(self.offset_owed and p in self.offset_owed["pairs"]))

    def drop_pair(self, p):
        if self.offset_owed and p in self.offset_owed["pairs"]:
            self.offset_owed = None
        if p.cause is not None and p.raised:
            self.event(f"stale_{p.kind}_{p.cause}")
        p.t.close()
        p.m.close()
        self.pairs.remove(p)

    def op_handles(self):
        """make, close and re-make filters and groupings; a stale one that has raised is replaced"""
        rng = self.rng
        done = False
        for p in [p for p in self.stale() if p.raised]:
            self.what += f" a {p.kind} stale by {p.cause} is re-made,"
            self.drop_pair(p)
            self.new_pair(p.kind)
            done = True
        for kind in ("filter", "grouping"):
            if not [p for p in self.pairs if p.kind == kind]:
                self.what += f" a first {kind},"
                self.new_pair(kind)
                done = True
        if done or self.n() == 0:
            return
        for p in [p for p in self.pairs if p.cause is None and not p.m.count()[0] and not self.owed(p)]:
            self.what += f" an empty {p.kind} goes"                        # (made while the index was empty)
            self.drop_pair(p)
            if not self.live(p.kind):
                self.new_pair(p.kind)
            done = True
        if done:
            return
        kind = "filter" if rng.random() < 0.5 else "grouping"
        live = self.live(kind)
        free = [p for p in live if not self.owed(p)]
        if free and (len(live) >= 2 or not free[0].m.count()[0]):
            self.what += f" close a {kind}, make another"
            self.drop_pair(free[0])
            if len(live) < 2:
                self.new_pair(kind)
        elif len(live) >= 2:
            self.what += " nothing to close"
        else:
            self.what += f" a second {kind}"
            self.new_pair(kind)

    # -- after every step -----------------------------------------------------------------------------------------------------------
    def check_state(self):
        t, m, rng = self.target, self.model, self.rng
        if len(t) != len(m) or t.removed != m.removed:
            self.fail(f"len {len(t)} removed {t.removed}, the model: len {len(m)} removed {m.removed}")
        Q = self.queries(2)
        sample = self.some_ids(40)
        valid_g = self.live("grouping")
        valid_f = self.live("filter")
        for p in list(self.pairs):
            if p.cause is not None:                                        # stale: every kind of call raises, until it is re-made
                one = np.array([[self.off() + 1, self.off() + 3]], dtype=np.uint64)
                if p.kind == "filter":
                    calls = [("allow ranges", lambda idx, f: f.allow(ranges=one)), ("deny ids", lambda idx, f: f.deny(ids=sample[:3])),
                             ("count", lambda idx, f: f.count()), ("ranges", lambda idx, f: f.ranges()),
                             ("search_with", lambda idx, f: idx.search_with(f, Q, 5))]
                    for name, fn in calls:
                        self.must_be_stale(f"stale filter ({p.cause}): {name}", fn, [p])
                    if valid_g:
                        self.must_be_stale(f"stale filter ({p.cause}): search_grouped", lambda idx, f, g: idx.search_grouped(g, Q, 5, flt=f),
                                           [p, valid_g[0]])
                else:
                    calls = [("set_ranges", lambda idx, g: g.set_ranges(one, 1)), ("set_ids", lambda idx, g: g.set_ids(sample[:3], 2)),
                             ("keys_of", lambda idx, g: g.keys_of(sample)), ("count", lambda idx, g: g.count()),
                             ("search_grouped", lambda idx, g: idx.search_grouped(g, Q, 5))]
                    for name, fn in calls:
                        self.must_be_stale(f"stale grouping ({p.cause}): {name}", fn, [p])
                    if valid_f:
                        self.must_be_stale(f"stale grouping ({p.cause}): search_grouped with a filter",
                                           lambda idx, g, f: idx.search_grouped(g, Q, 5, flt=f), [p, valid_f[0]])
                p.raised = True
            elif p.kind == "filter":
                if p.t.count() != p.m.count():
                    self.fail(f"filter count {p.t.count()}, the model {p.m.count()}")
                if not np.array_equal(p.t.ranges(), p.m.ranges()):
                    self.fail("filter ranges differ from the model's")
            else:
                if p.t.count() != p.m.count():
                    self.fail(f"grouping count {p.t.count()}, the model {p.m.count()}")
                if not np.array_equal(p.t.keys_of(sample), p.m.keys_of(sample)):
                    self.fail("grouping keys_of differs from the model's")

    # -- the checked calls ------------------------------------------------------------------------------------------------------------
    def choose_forms(self):
        rng = self.rng
        have_f, have_g = bool(self.live("filter")), bool(self.live("grouping"))
        ok = [f for f in FORMS if not (f == "with" and not have_f) and not (f == "grouped" and not have_g)
              and not (f == "grouped_f" and not (have_f and have_g))]
        forms = [f for f in dict.fromkeys(self.forced) if f in ok]
        self.forced = []
        rest = [f for f in ok if f not in forms]
        rest = [rest[i] for i in rng.permutation(len(rest))]
        forms += rest[:max(0, int(rng.integers(4, 7)) - len(forms))]
        if not set(forms) & set(SHARED):
            forms.append(next(f for f in rest if f in SHARED))
        return [forms[i] for i in rng.permutation(len(forms))]

    def check_calls(self):
        forms = self.choose_forms()
        for j, form in enumerate(forms):
            if j == 1 and self.copy_pending:
                self.target.set_filter_copy(self.copy_pending)
                self.model.set_filter_copy(self.copy_pending)
                self.copy_pending = None
                self.event("copy_switch_between_forms")
            getattr(self, "form_" + form)()

    def checked(self, form, call, fn, pairs=()):
        call = f"{form}({call})"
        want, got = self.both(call, fn, pairs)
        if want[0] == "ok":
            self.same(call, got[1], want[1], FIELDS[form])
        return want

    def pick_of(self, values):
        return values[int(self.rng.integers(0, len(values)))]

    def form_search(self):
        B, k = int(self.rng.integers(1, 7)), self.pick_of((1, 10, 64, 100, 300))
        Q = self.queries(B)
        self.checked("search", f"B={B}, k={k}", lambda idx: idx.search(Q, k))
        self.note_path("search", k)

    def form_filtered(self):
        rng = self.rng
        B, k = int(rng.integers(1, 7)), self.pick_of((1, 10, 70))
        Q = self.queries(B)
        if rng.random() < 0.5:
            r = self.random_ranges(int(rng.integers(0, 5)))
            self.checked("filtered", f"B={B}, k={k}, {len(r)} ranges", lambda idx: idx.search_filtered(Q, k, ranges=r))
        else:
            ids = self.some_ids(int(rng.integers(1, 300)))
            self.checked("filtered", f"B={B}, k={k}, {len(ids)} ids", lambda idx: idx.search_filtered(Q, k, ids=ids))

    def form_with(self):
        B, k = int(self.rng.integers(1, 7)), self.pick_of((1, 10, 70, 300))
        Q = self.queries(B)
        p = self.pick_pair("filter")
        self.checked("with", f"B={B}, k={k}", lambda idx, f: idx.search_with(f, Q, k), [p])
        self.note_path("with", k)
        self.note_handles_searched("with", [p])

    def thresholds(self, B):
        return self.rng.choice(np.array([-1.0, 0.0, 0.05, 0.1, 0.3, 0.9, 0.999, 1.5], dtype=np.float32), B)

    def form_range(self):
        B, cap = int(self.rng.integers(1, 7)), self.pick_of((1, 8, 64, 300, 4096))
        Q, t = self.queries(B), self.thresholds(B)
        self.checked("range", f"B={B}, cap={cap}, thresholds {t.tolist()}", lambda idx: idx.search_range(Q, t, cap))

    def form_mmr(self):
        B, k = int(self.rng.integers(1, 7)), self.pick_of((1, 5, 10))
        fetch, lam = self.pick_fetch("mmr", k, (k, 32, 64, 300)), self.pick_of((0.3, 0.5, 0.7, 1.0))
        Q = self.queries(B)
        self.checked("mmr", f"B={B}, k={k}, fetch={fetch}, lam={lam}", lambda idx: idx.search_mmr(Q, k, fetch=fetch, lam=lam))
        self.note_fetch("mmr", fetch)
        self.note_path("mmr", fetch)

    def form_fused(self):
        rng = self.rng
        R, m, k = int(rng.integers(1, 4)), self.pick_of((1, 3, 16)), self.pick_of((1, 10, 40))
        mode = self.pick_of(("max", "rrf"))
        fetch = self.pick_fetch("fused", k, (k, 32, 64) if mode == "max" else (k, 32, 64, 256))
        Q = self.queries(R * m).reshape(R, m, self.d)
        W = None
        if rng.random() < 0.7:
            W = rng.uniform(0.5, 2.0, (R, m)).astype(np.float32)
            W[rng.random((R, m)) < 0.3] = 0.0                              # absent sub-queries
        self.checked("fused", f"R={R}, m={m}, k={k}, {mode}, fetch={fetch}, weights {None if W is None else W.tolist()}",
                     lambda idx: idx.search_fused(Q, k, mode=mode, fetch=fetch, weights=W))
        self.note_fetch("fused", fetch)

    def grouped(self, form, flt):
        B, k = int(self.rng.integers(1, 7)), self.pick_of((1, 5, 10, 20))
        fetch = self.pick_fetch(form, k, (k, 16, 64, 300))
        if flt is not None and flt is self.document:                       # fewer groups than k in fewer rows than fetch
            k, fetch, self.document = self.pick_of((5, 10)), self.pick_of((64, 300)), None
        Q = self.queries(B)
        g = self.pick_pair("grouping")
        if flt is None:
            self.checked(form, f"B={B}, k={k}, fetch={fetch}", lambda idx, g_: idx.search_grouped(g_, Q, k, fetch=fetch), [g])
        else:
            want = self.checked(form, f"B={B}, k={k}, fetch={fetch}, filter of {flt.m.count()[0]}",
                                lambda idx, g_, f_: idx.search_grouped(g_, Q, k, fetch=fetch, flt=f_), [g, flt])
            if want[0] == "ok" and k <= flt.m.count()[1] < fetch and (want[1][5] < k).any():
                self.event("complete_by_short_list")
        self.note_fetch(form, fetch)
        self.note_path("grouped", fetch)
        self.note_handles_searched(form, [g] + ([flt] if flt is not None else []))

    def form_grouped(self):
        self.grouped("grouped", None)

    def form_grouped_f(self):
        self.grouped("grouped_f", self.pick_pair("filter"))

    def form_by_id(self):
        B, e = int(self.rng.integers(1, 7)), bool(self.rng.random() < 0.5)
        k = self.pick_width("by_id", (1, 10, 70, 256), int(e))
        ids = self.query_ids("by_id", B)
        self.checked("by_id", f"ids {ids.tolist()}, k={k}, exclude_self={e}", lambda idx: idx.search_by_id(ids, k, exclude_self=e))
        self.note_named("by_id", ids)
        self.note_width("by_id", k + e)
        self.note_path("by_id", k + e)

    def form_range_by_id(self):
        B, cap, e = int(self.rng.integers(1, 7)), self.pick_of((1, 8, 64, 256)), bool(self.rng.random() < 0.6)
        ids, t = self.query_ids("range_by_id", B), self.thresholds(B)
        self.checked("range_by_id", f"ids {ids.tolist()}, thresholds {t.tolist()}, cap={cap}, exclude_self={e}",
                     lambda idx: idx.search_range_by_id(ids, t, cap, exclude_self=e))

    def form_like(self):
        rng = self.rng
        R, m, e = int(rng.integers(1, 4)), self.pick_of((1, 3, 8, 16)), bool(rng.random() < 0.6)
        k = self.pick_width("like", (5, 60, 250), m if e else 0)
        ex = self.some_ids(R * m).reshape(R, m)
        zero = np.flatnonzero(~self.model.rows.any(axis=1))
        if zero.size and m > 1:
            ex[0, -1] = int(zero[int(rng.integers(0, zero.size))]) + 1 + self.off()          # a zero row
        if m > 2:
            ex[-1, 1] = ex[-1, 0]                                                             # an id named twice
        dead = np.flatnonzero(~self.model.alive)
        if dead.size:
            ex[0, 0] = int(dead[int(rng.integers(0, dead.size))]) + 1 + self.off()              # a removed row
        self.name_marked(ex, (0, 0))
        self.name_moved("like", ex, (R - 1, m - 1) if R > 1 else (0, 0))
        W = None
        if rng.random() < 0.6:
            W = (rng.uniform(0.25, 2.0, (R, m)) * rng.choice([1.0, 1.0, -0.5], (R, m))).astype(np.float32)
            W[rng.random((R, m)) < 0.15] = 0.0
        Q = qw = None
        if rng.random() < 0.5:
            Q = self.queries(R)
            qw = None if rng.random() < 0.5 else rng.uniform(0.5, 1.5, R).astype(np.float32)
        self.checked("like", f"examples {ex.tolist()}, k={k}, weights {None if W is None else W.tolist()}, "
                     f"{'no ' if Q is None else ''}caller vector, exclude_examples={e}",
                     lambda idx: idx.search_like(ex, k, weights=W, queries=Q, query_weights=qw, exclude_examples=e))
        self.note_named("like", ex)
        self.note_width("like", k + (m if e else 0))
        self.note_path("like", k + (m if e else 0))

    def form_score_ids(self):
        B, m = int(self.rng.integers(1, 7)), self.pick_width("score_ids", (1, 8, 70, 1025))
        Q = self.queries(B)
        ids = self.some_ids(B * m).reshape(B, m)
        if m > 2:
            ids[:, 1] = ids[:, 0]                                                             # a repeat
            ids[0, 2] = 0
        self.name_marked(ids, (B - 1, m - 1))
        self.name_moved("score_ids", ids, (0, 0))
        self.checked("score_ids", f"B={B}, m={m}", lambda idx: idx.score_ids(Q, ids))
        self.note_named("score_ids", ids)
        self.note_width("score_ids", m)

    # -- one step -------------------------------------------------------------------------------------------------------------------
    def step(self, i):
        self.step_no = i
        op = self.pick()
        self.what = f"{self.tag} step {i}: {op}"
        getattr(self, "op_" + op)()
        self.log.append(self.what)
        self.check_state()
        self.check_calls()
        if self.exact_step:                                                # EXACT for one step only
            self.target.set_search_mode(0)
            self.model.set_search_mode(0)
            self.exact_step = False

    def close(self):
        for p in list(self.pairs):
            p.t.close()
            p.m.close()
        self.pairs = []


def run(target, model, rng, steps, on_event=None, store_dir="store", cone=False, tag="walk", shards=1, block_rows=0):
    """the walk; raises AssertionError naming tag (the seed), the step and the operation at the first difference.  shards and
    block_rows say how the target deals its rows to shards (a plain index: 1, 0): the capacities the growth events are about are
    each shard's own"""
    w = Walk(target, model, rng, on_event, store_dir, cone, tag, shards, block_rows)
    try:
        for i in range(steps):
            w.step(i)
    finally:
        w.close()
    return w
