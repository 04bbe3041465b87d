"""The contract of grouped search with members (mx_index_search_group_rows, mx_index_search_capped, mx_grouping_key_counts, DESIGN.md
section 3.19) restated in NumPy -- TEST INFRASTRUCTURE, not product code.  Built on the candidate lists and keys of grouped_model.py.

    list L      what the candidate stage gives: the exact top-fetch in (dist, id) order over the live (and allowed) rows
    head        an entry whose key is 0, or whose key no earlier entry of L has; the first k heads are reported in list order

    group rows  slot [j, r] of head j with key K != 0: the r-th entry of L with key K (r < n; slot 0 is the head); a key-0 head has
                itself only.  group_rows = entries of L under K (1 for key 0); n_members = min(n, group_rows); blanks id 0 / score 0 /
                dist +inf (key 0, group_rows 0, n_members 0, members_complete 0 behind the heads found).
                members_complete = n_members == n, or |L| < fetch, or key 0;  complete = n_found == k, or |L| < fetch

    capped      an entry is accepted when its key is 0 or fewer than per_key earlier entries of L have its key; the first k accepted
                entries unchanged, with their key;  complete = n_found == k, or |L| < fetch
"""
import numpy as np

from grouped_model import candidate_lists, row_keys


def default_fetch_rows(k, n):
    return min(4096, max(k, min(256, max(32, 4 * k * n))))


def entry_keys(ids, m, keys, id_offset=0):
    """the keys of the first m entries of one list (ids under id_offset; keys per global row)"""
    r = np.asarray(ids[:m]).astype(np.int64) - 1 - id_offset
    ek = np.zeros(m, np.uint32)
    inside = (r >= 0) & (r < keys.size)
    ek[inside] = keys[r[inside]]
    return ek


def group_rows_list(ids, scores, dists, m, ekeys, k, n, fetch):
    """one query's list (m entries) and the keys of its entries -> (ids [k, n], scores [k, n], dists [k, n], keys [k], group_rows [k],
    n_members [k], members_complete [k], n_found, complete)"""
    oi = np.zeros((k, n), np.uint64)
    osc = np.zeros((k, n), np.float32)
    od = np.full((k, n), np.inf, np.float32)
    ok = np.zeros(k, np.uint32)
    orows = np.zeros(k, np.int32)
    omem = np.zeros(k, np.int32)
    omc = np.zeros(k, bool)
    head_of = {}                                                           # key -> its head's number
    heads = 0
    for j in range(m):
        key = int(ekeys[j])
        if key != 0 and key in head_of:
            h = head_of[key]
            if h < k:
                orows[h] += 1
                if omem[h] < n:
                    oi[h, omem[h]], osc[h, omem[h]], od[h, omem[h]] = ids[j], scores[j], dists[j]
                    omem[h] += 1
            continue
        if key != 0:
            head_of[key] = heads
        if heads < k:
            oi[heads, 0], osc[heads, 0], od[heads, 0], ok[heads] = ids[j], scores[j], dists[j], key
            orows[heads] = omem[heads] = 1
        heads += 1
    nf = min(k, heads)
    for h in range(nf):
        omc[h] = bool(omem[h] == n or m < fetch or ok[h] == 0)
    return oi, osc, od, ok, orows, omem, omc, nf, bool(nf == k or m < fetch)


def capped_list(ids, scores, dists, m, ekeys, k, per_key, fetch):
    """-> (ids [k], scores [k], dists [k], keys [k], n_found, complete)"""
    oi = np.zeros(k, np.uint64)
    osc = np.zeros(k, np.float32)
    od = np.full(k, np.inf, np.float32)
    ok = np.zeros(k, np.uint32)
    seen = {}
    nf = 0
    for j in range(m):
        key = int(ekeys[j])
        if key != 0:
            before = seen.get(key, 0)
            seen[key] = before + 1
            if before >= per_key:
                continue
        if nf < k:
            oi[nf], osc[nf], od[nf], ok[nf] = ids[j], scores[j], dists[j], key
            nf += 1
        if nf == k:
            break
    return oi, osc, od, ok, nf, bool(nf == k or m < fetch)


def _stack(out, i, shape, dtype):
    return np.stack([o[i] for o in out]) if out else np.zeros(shape, dtype)


def group_rows_lists(ci, cs, cd, cnf, keys, k, n, fetch, id_offset=0):
    """lists [B, fetch] and the keys per global row -> what FlatIndex.search_group_rows returns: (ids, scores, dists [B, k, n], keys,
    group_rows, n_members, members_complete [B, k], n_found, complete [B])"""
    keys = np.asarray(keys, np.uint32)
    out = [group_rows_list(ci[b], cs[b], cd[b], int(cnf[b]), entry_keys(ci[b], int(cnf[b]), keys, id_offset), k, n, fetch)
           for b in range(ci.shape[0])]
    return (_stack(out, 0, (0, k, n), np.uint64), _stack(out, 1, (0, k, n), np.float32), _stack(out, 2, (0, k, n), np.float32),
            _stack(out, 3, (0, k), np.uint32), _stack(out, 4, (0, k), np.int32), _stack(out, 5, (0, k), np.int32),
            _stack(out, 6, (0, k), bool), np.asarray([o[7] for o in out], np.int32), np.asarray([o[8] for o in out], bool))


def capped_lists(ci, cs, cd, cnf, keys, k, per_key, fetch, id_offset=0):
    """-> what FlatIndex.search_capped returns: (ids, scores, dists, keys [B, k], n_found, complete [B])"""
    keys = np.asarray(keys, np.uint32)
    out = [capped_list(ci[b], cs[b], cd[b], int(cnf[b]), entry_keys(ci[b], int(cnf[b]), keys, id_offset), k, per_key, fetch)
           for b in range(ci.shape[0])]
    return (_stack(out, 0, (0, k), np.uint64), _stack(out, 1, (0, k), np.float32), _stack(out, 2, (0, k), np.float32),
            _stack(out, 3, (0, k), np.uint32), np.asarray([o[4] for o in out], np.int32), np.asarray([o[5] for o in out], bool))


def group_rows_model(oracle, rows, Q, k, n, keys, fetch=None, alive=None, allowed=None, id_offset=0):
    fetch = default_fetch_rows(k, n) if fetch is None else fetch
    ci, cs, cd, cnf = candidate_lists(oracle, rows, Q, fetch, alive, allowed, id_offset)
    return group_rows_lists(ci, cs, cd, cnf, row_keys(keys, np.asarray(rows).shape[0]), k, n, fetch, id_offset)


def capped_model(oracle, rows, Q, k, per_key, keys, fetch, alive=None, allowed=None, id_offset=0):
    ci, cs, cd, cnf = candidate_lists(oracle, rows, Q, fetch, alive, allowed, id_offset)
    return capped_lists(ci, cs, cd, cnf, row_keys(keys, np.asarray(rows).shape[0]), k, per_key, fetch, id_offset)


def key_counts_model(keys, n_rows, asked, alive=None):
    """keys per global row (possibly shorter than the rows), asked [m] -> (rows under each asked key, those of them not removed)"""
    rk = row_keys(keys, n_rows)
    live = np.ones(n_rows, bool) if alive is None else np.asarray(alive, bool)[:n_rows]
    asked = np.asarray(asked, np.uint32).reshape(-1)
    return (np.asarray([int((rk == a).sum()) for a in asked], np.uint64),
            np.asarray([int(((rk == a) & live).sum()) for a in asked], np.uint64))


def settle_model(out_keys, n_members, members_complete, n_found, keys, n_rows, alive=None):
    """members_complete after settle=True: raised where the flag is 0 and n_members equals the key's live rows"""
    mc = np.array(members_complete, bool)
    rk = row_keys(keys, n_rows)
    live = np.ones(n_rows, bool) if alive is None else np.asarray(alive, bool)[:n_rows]
    for b in range(mc.shape[0]):
        for j in range(int(n_found[b])):
            if not mc[b, j] and int(n_members[b, j]) == int(((rk == out_keys[b, j]) & live).sum()):
                mc[b, j] = True
    return mc


# ---- brute force over all rows: what the flags are held to -------------------------------------------------------------------------
def full_order(oracle, rows, q, alive=None, allowed=None):
    """every live (and allowed) row with a non-NaN dist in (dist, id) order -> (rows [n], dists of all rows)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    d = oracle.all_dists(rows, np.ascontiguousarray(q, dtype=np.float32))
    ok = np.ones(rows.shape[0], bool)
    if alive is not None:
        ok &= np.asarray(alive, bool)
    if allowed is not None:
        ok &= np.asarray(allowed, bool)
    order = sorted((r for r in range(rows.shape[0]) if ok[r] and d[r] == d[r]), key=lambda r: (float(d[r]), r))
    return np.asarray(order, np.int64), d


def brute_group_members(order, rk, k):
    """the walk over the full order: the first k heads, and for each EVERY row of its group in order -> [(key, [rows])]"""
    groups, at = [], {}
    for r in order.tolist():
        key = int(rk[r])
        if key != 0 and key in at:
            if at[key] < k:
                groups[at[key]][1].append(r)
            continue
        if key != 0:
            at[key] = len(groups)
        groups.append((key, [r]))
    return groups[:k]


def brute_capped(order, rk, k, per_key):
    """the walk over the full order -> the first k accepted rows"""
    seen, acc = {}, []
    for r in order.tolist():
        key = int(rk[r])
        if key != 0:
            before = seen.get(key, 0)
            seen[key] = before + 1
            if before >= per_key:
                continue
        acc.append(r)
        if len(acc) == k:
            break
    return acc
