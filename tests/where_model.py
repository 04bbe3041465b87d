"""The contract of the filters built from row attributes (mx_filter_set_where, mx_filter_set_keys, mx_filter_combine,
mx_filter_invert) restated in NumPy on boolean arrays -- TEST INFRASTRUCTURE, not product code.

A filter is a boolean per global row, as in filtered_model.py.  A prior is an f32 per row and a grouping a u32 per row, both 0 where
nothing was set and for rows the column does not reach.
"""
import numpy as np

AND, OR, ANDNOT, XOR = 0, 1, 2, 3
OPS = {"and": AND, "or": OR, "andnot": ANDNOT, "xor": XOR}


def column(values, n, dtype):
    """the column as the kernels read it: `values` for the rows it covers, 0 from there on, n rows"""
    c = np.zeros(n, dtype=dtype)
    v = np.asarray(values, dtype=dtype).reshape(-1)[:n]
    c[: v.size] = v
    return c


def select_where(values, n, lo, hi):
    """bool [n]: lo <= v && v <= hi in IEEE f32 (NaN bounds are refused before this is asked)"""
    v = column(values, n, np.float32)
    return (np.float32(lo) <= v) & (v <= np.float32(hi))


def select_keys(keys, n, wanted):
    """bool [n]: the row's key is one of `wanted` (any order, repeats allowed; key 0 = the ungrouped rows)"""
    return np.isin(column(keys, n, np.uint32), np.asarray(list(wanted), dtype=np.uint32))


def edit(model, selection, allow):
    """allow = 1 adds the selection to the set, allow = 0 takes it away -> (new model, n_selected)"""
    return (model | selection) if allow else (model & ~selection), int(selection.sum())


def combine(a, b, op):
    op = OPS.get(op, op)
    if op == AND:
        return a & b
    if op == OR:
        return a | b
    if op == ANDNOT:
        return a & ~b
    if op == XOR:
        return a ^ b
    raise ValueError(op)


def invert(a):
    return ~a


def grown(a, n):
    """a filter made when the index held fewer rows: the rows appended since are outside the set"""
    out = np.zeros(n, dtype=bool)
    out[: a.size] = a
    return out
