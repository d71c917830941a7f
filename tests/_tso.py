"""Expected frames of segmentation offload on the transmit pass (nsx_tso_ipv4_tcp_build_* / nsx_tso_ipv6_tcp_build_*),
on the CPU.

A super-segment batch is expanded here, in numpy, into the per-frame batch a caller without the offload would have
to make (a tests/_tx.Case: repeated fields, the repeated option bytes materialised, the slice boundaries as data_off,
seq / control / ident per the rules of include/nsx_csum.h), and tests/_tx.expected is called on that — so the expected
bytes come from the Go-faithful sender loop that pins the transmit pass. tests/test_tso_abi.py holds the expansion to
O.ipv4_tcp_frame / O.ipv6_tcp_frame frame by frame and to the receive oracle."""
import numpy as np

import _tx

FIN, PSH, CWR = 0x01, 0x08, 0x80
LAST_ONLY, FIRST_ONLY = FIN | PSH, CWR  # Linux tcp_gso_segment: FIN / PSH on the last frame, CWR on the first


class Batch:
    """n super-segments: a tests/_tx.Case whose every entry is one super-segment (`sup`: fields, options, payload
    runs, IP fields) and mss[s], the payload bytes per frame."""

    def __init__(self, rng, ipver, lens, mss, opts=None, lead=0):
        self.sup = _tx.Case(rng, ipver, lens, opts=opts, lead=lead)
        self.ipver, self.n = ipver, self.sup.n
        self.mss = np.broadcast_to(np.asarray(mss, np.uint32), self.n).copy()
        self.first = count(self.sup.data_off, self.mss)
        self.seg, self.off = layout(self.sup.data_off, self.mss, self.first, self.sup.opt_off, _tx.IPH[ipver])
        self.nf = int(self.first[-1])


def count(data_off, mss):
    """nsx_tso_count_host restated: frame_first = the prefix sum of max(1, ceil(len_s / mss_s))."""
    lens = np.diff(np.asarray(data_off, np.uint64)).astype(np.uint64)
    mss = np.asarray(mss, np.uint64)[:lens.size]
    cnt = np.maximum((lens + mss - np.uint64(1)) // mss, np.uint64(1))
    first = np.zeros(lens.size + 1, np.uint64)
    first[1:] = np.cumsum(cnt)
    return first


def frame_index(first):
    """(frame_seg, j): each frame's super-segment and its index in it."""
    first = np.asarray(first, np.uint64)
    cnt = np.diff(first).astype(np.int64)
    seg = np.repeat(np.arange(cnt.size, dtype=np.int64), cnt)
    j = np.arange(int(first[-1]), dtype=np.int64) - first[:-1].astype(np.int64)[seg]
    return seg, j


def slices(data_off, mss, first):
    """(start, end) of every frame's payload slice in the data array."""
    data_off = np.asarray(data_off, np.uint64).astype(np.int64)
    seg, j = frame_index(first)
    m = np.asarray(mss, np.int64)[seg]
    lo = np.minimum(data_off[:-1][seg] + j * m, data_off[1:][seg])
    return lo, np.minimum(lo + m, data_off[1:][seg])


def layout(data_off, mss, first, opt_off=None, ip_hdr_len=20):
    """nsx_tso_layout_host restated: (frame_seg u32, out_off u64) — packed round_up4(ip_hdr_len + wire) slots."""
    seg, _ = frame_index(first)
    lo, hi = slices(data_off, mss, first)
    olen = np.zeros(seg.size, np.uint64) if opt_off is None else np.diff(np.asarray(opt_off, np.uint64))[seg]
    flen = _tx.wire_len(olen, (hi - lo).astype(np.uint64)) + np.uint64(ip_hdr_len)
    off = np.zeros(seg.size + 1, np.uint64)
    off[1:] = np.cumsum((flen + np.uint64(3)) & ~np.uint64(3))
    return seg.astype(np.uint32), off


def expand(b, null=()):
    """The per-frame tests/_tx.Case of batch b. null: the optional arrays passed as NULL ("ident": 0 + j; "ttl": 64;
    "tclass" / "flow": 0; "offset" needs nothing — the case's array already holds computeOffset())."""
    s = b.sup
    seg, j = frame_index(b.first)
    lo, hi = slices(s.data_off, b.mss, b.first)
    last = j == (np.diff(b.first).astype(np.int64)[seg] - 1)
    c = _tx.Case.__new__(_tx.Case)
    c.ipver, c.n = b.ipver, seg.size
    c.data = s.data
    # consecutive slices share their boundary (a Case packs its payload runs), so the cut points are one offsets array
    assert np.array_equal(lo[1:], hi[:-1])
    c.data_off = np.concatenate([lo, hi[-1:]]).astype(np.uint64)
    c.fields = {k: np.ascontiguousarray(v[seg]) for k, v in s.fields.items()}
    m = np.asarray(b.mss, np.uint64)[seg]
    c.fields["seq_num"] = ((s.fields["seq_num"][seg].astype(np.uint64) + j.astype(np.uint64) * m)
                           & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctl = s.fields["control"][seg].astype(np.uint8)
    ctl = np.where(last, ctl, ctl & np.uint8(0xFF ^ LAST_ONLY))
    c.fields["control"] = np.where(j == 0, ctl, ctl & np.uint8(0xFF ^ FIRST_ONLY)).astype(np.uint8)
    c.opts = c.opt_off = None
    olen = np.zeros(seg.size, np.uint64)
    if s.opt_off is not None:
        ob = [s.opts[int(s.opt_off[i]):int(s.opt_off[i + 1])].tobytes() for i in seg]
        olen = np.array([len(x) for x in ob], np.uint64)
        c.opts = np.frombuffer(b"\x77" + b"".join(ob) + b"\x77", np.uint8).copy()
        c.opt_off = np.zeros(seg.size + 1, np.uint64)
        c.opt_off[1:] = np.cumsum(olen)
        c.opt_off += np.uint64(1)
    c.wire = _tx.wire_len(olen, (hi - lo).astype(np.uint64))
    c.flen = c.wire + np.uint64(_tx.IPH[b.ipver])
    c.ip = {k: np.ascontiguousarray(v[seg]) for k, v in s.ip.items()}
    ident = np.zeros(seg.size, np.uint64) if "ident" in null else c.ip["ident"].astype(np.uint64)
    c.ip["ident"] = ((ident + j.astype(np.uint64)) & np.uint64(0xFFFF)).astype(np.uint16)
    if "ttl" in null:
        c.ip["ttl"] = np.full(seg.size, 64, np.uint8)
    for k in ("tclass", "flow"):
        if k in null:
            c.ip[k] = np.zeros_like(c.ip[k])
    return c


def expected(b, off=None, fill=0, null=()):
    """The output buffer and the per-frame TCP raw sums the offload must produce for frames at off[f] (default: the
    packed layout) over a buffer pre-filled with `fill`; tests/_tx.expected over the expanded batch. Returns (buf,
    raw, case) — the expanded case for messages and for the plain transmit pass."""
    c = expand(b, null)
    buf, raw = _tx.expected(c, b.off if off is None else off, fill=fill)
    return buf, raw, c
