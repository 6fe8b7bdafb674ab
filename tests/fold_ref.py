"""Brute-force restatement of wavenet_amd/fold.py for the tests: everything position by position, nothing shared with the module.

A plan is four lists (a, b, s, e).  Columns are found by walking every window-inclusive position a segment touches and asking
the alignment rule which columns it reads.  The signal is built one sample at a time with numpy float32 scalars."""
import numpy as np


def plan(n, B, O, W):
    """Bodies of B from 0 on; the last one swallows a rest of at most O samples."""
    S = 1
    while n - S * B > O:
        S += 1
    a = [u * B for u in range(S)]
    b = a[1:] + [n]
    s = [0] + [max(0, a[u] - W) for u in range(1, S)]
    e = [b[u] + O for u in range(S - 1)] + [n]
    return a, b, s, e


def covers(n, B, O, W):
    """Per position: the segments that decode it outside their warm-up, and its owners (bodies holding it)."""
    a, b, s, e = plan(n, B, O, W)
    decoded = [[u for u in range(len(a)) if a[u] <= p < e[u]] for p in range(n)]
    owners = [[u for u in range(len(a)) if a[u] <= p < b[u]] for p in range(n)]
    return decoded, owners


def columns_read(s, e, window, phase, hop, interp, upsample=1):
    """The coarse columns of the utterance that a segment decoding [s, e) touches: its window starts at window-inclusive index s
    and it runs over window + (e - s) - 1 positions (the last emitted sample is never fed back).  Position t reads fine column
    (t + phase) // hop' -- and the next one under linear interpolation --; fine column m of a learned layer is made from the
    coarse columns m // U and m // U + 1."""
    fine = hop // upsample
    cols = set()
    for t in range(s, s + window + (e - s) - 1):
        m = (t + phase) // fine
        for mm in ([m, m + 1] if interp == "linear" else [m]):
            cols.update([mm] if upsample == 1 else [mm // upsample, mm // upsample + 1])
    return sorted(cols)


def unfold(rows, n, B, O, W, table):
    a, b, s, e = plan(n, B, O, W)
    out = np.zeros((n,), np.int16)
    for p in range(n):
        u = [k for k in range(len(a)) if a[k] <= p < b[k]][0]
        seam = [k for k in range(len(a) - 1) if b[k] <= p < b[k] + O]
        if not seam:
            out[p] = table[rows[u][p - s[u]]]
            continue
        k = seam[0]
        t = np.float32(table[rows[k][p - s[k]]])
        h = np.float32(table[rows[k + 1][p - s[k + 1]]])
        w = np.float32((p - b[k] + 0.5) / O)
        d = np.float32(h - t)
        m = np.float32(w * d)
        y = float(np.float32(t + m))
        r = np.floor(y)
        if y - r > 0.5 or (y - r == 0.5 and r % 2 == 1):           # round half to even
            r += 1
        out[p] = int(min(max(r, -32768), 32767))
    return out
