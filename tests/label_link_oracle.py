"""Oracle of gim_amd/video_labels.py and ops.label_link: the reference's formulation of `link` and `propagate`
(datasets/walk/walk.py:29,170-247) -- a dict per side from rounded pixel key to the last row that has it, the set of shared keys, the
unique (i, j) columns in sorted order, and a sequential recursion over hops that keeps a list of at most two labels and the list of
frame ids they span.  Written independently of the code under test (which uses tables over the key range and a carried label);
numpy and Python containers only."""
import numpy as np


def last_row_by_key(xs, ys, width):
    """{key: row}: key = round(x) + round(y) * width in the arrays' fp32; a later row replaces an earlier one of the same key"""
    keys = np.round(xs) + np.round(ys) * width
    assert keys.dtype == np.float32
    table = {}
    for row, key in enumerate(keys.tolist()):
        table[key] = row
    return table


def link_ij(label0, label1, width):
    """the joined rows -> int64 [2, n]: for every key both sides have, (its row in label0, its row in label1); duplicates removed,
    columns in lexicographic order (what np.unique(..., axis=1) returns)"""
    rows0 = last_row_by_key(label0[:, 2], label0[:, 3], width)
    rows1 = last_row_by_key(label1[:, 0], label1[:, 1], width)
    columns = sorted({(rows0[key], rows1[key]) for key in set(rows0) & set(rows1)})
    return np.array(columns, dtype=np.int64).reshape(-1, 2).T


def link(label0, label1, width, min_final_matches):
    i, j = link_ij(label0, label1, width)
    if len(i) < min_final_matches:
        return None
    return np.concatenate([label0[i, :2], label1[j, 2:]], axis=1)


class Walk:
    """propagate over labels held in memory: labels[skip][(idx0, idx1)] = [one array per source].  `trace` records the branches taken
    ("fallback": a failed link shortened the hop; "none": a call returned nothing)."""

    def __init__(self, labels, width, min_final_matches):
        self.labels, self.width, self.min_final_matches = labels, width, min_final_matches
        self.trace = []

    def dump(self, skip, pair):
        sources = self.labels.get(skip, {}).get((int(pair[0]), int(pair[1])), [])
        return np.concatenate(sources, axis=0).astype(np.float32) if sources else []

    def propagate(self, idx0, idx1, skips):
        stride, shorter = skips[-1], skips[:-1]
        stops = [idx0] + [idx0 + stride * (k + 1) for k in range((idx1 - idx0) // stride)]
        if stops[-1] != idx1:
            stops.append(idx1)
        todo = [(stops[k], stops[k + 1]) for k in range(len(stops) - 1)]
        held, frames = [], [idx0]                 # the labels not yet linked (at most two) and the frame ids they span
        while todo:
            first, last = todo.pop(0)
            if first == last:
                break
            found = []
            if last - first == stride:
                direct = self.dump(stride, (first, last))
                if len(direct) > 0:
                    found.append(direct)
            if shorter:
                sub, sub0, sub1 = self.propagate(first, last, shorter)
                if (sub0, sub1) == (first, last):
                    found.append(sub)
            if found:
                held.append(np.concatenate(found, axis=0))
                frames.append(last)
            if len(held) == 2:
                joined = link(held[0], held[1], self.width, self.min_final_matches)
                if joined is None:
                    held.pop()
                    frames.pop()
                    todo = [(first, last - skips[0])]
                    self.trace.append("fallback")
                else:
                    held, frames = [joined], [frames[0], frames[-1]]
        if len(held) == 1 and len(frames) == 2:
            return held[0], frames[0], frames[1]
        self.trace.append("none")
        return None, None, None
