"""Shared helpers of the fragmentation / reassembly GPU tests (tests/test_gpu_frag.py, tests/test_gpu_reasm.py,
tests/test_gpu_frag_fuzz.py): one device call over outputs pre-filled with a fill byte, the model's outputs
(tests/_frag.py) laid into arrays filled the same way, and their comparison array for array — so every region that must
stay untouched is compared too."""
import numpy as np

import _frag as F
import _gro_gpu
from _gpu import host, torch, nsx

FILL = _gro_gpu.FILL
_NP = _gro_gpu._NP
d = _gro_gpu.d
same = _gro_gpu.same
GUARD = 64


# ------------------------------------------------------------------ fragmentation
def frag_map(offs, mtu):
    """The host helpers' frame map as (first, src, out_off) numpy arrays."""
    first = nsx.frag_count_host(offs, mtu)
    src, off = nsx.frag_layout_host(offs, mtu, first)
    return first, src, off


def frag_gpu(buf, offs, mtu, tune=None, dlead=0, d_buf=None, d_offs=None):
    """One device call: (the output buffer with GUARD sentinel bytes of FILL on either side of the slots, status). The
    slots start dlead bytes into a 256-aligned allocation's 64th byte, so dlead is the destination alignment."""
    mtu = np.ascontiguousarray(np.broadcast_to(np.asarray(mtu, np.uint32), offs.size - 1))
    first, src, off = frag_map(offs, mtu)
    total = int(off[-1])
    arena = torch.full((GUARD + dlead + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    n = offs.size - 1
    status = torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda")
    got = nsx.frag_ipv4_dev(d(buf) if d_buf is None else d_buf, d(offs) if d_offs is None else d_offs, d(mtu),
                            d(first), d(src if src.size else np.zeros(1, np.uint32)), arena[GUARD + dlead:], d(off),
                            status=status, tune=tune, n_frags=src.size)
    assert got is status
    a = host(arena)
    assert (a[:dlead] == FILL).all()
    return a[dlead:], host(status)


def frag_want(buf, offs, mtu):
    mtu = np.broadcast_to(np.asarray(mtu, np.uint32), offs.size - 1)
    out, off, first, src, status = F.frag(buf, offs, mtu, fill=FILL)
    w = np.full(GUARD + out.size + GUARD, FILL, np.uint8)
    w[GUARD:GUARD + out.size] = out
    st = np.full(max(status.size, 1), FILL, np.uint8)
    st[:status.size] = status
    return w, st, off


def frag_check(buf, offs, mtu, tunes=(None,), dleads=(0,), what=""):
    """The device against the model over every tune and destination alignment given; returns (status, out_off, the
    model's output bytes without the sentinels)."""
    w, st, off = frag_want(buf, offs, mtu)
    for tune in tunes:
        for dlead in dleads:
            got, gst = frag_gpu(buf, offs, mtu, tune=tune, dlead=dlead)
            assert np.array_equal(gst, st), f"{what} tune={tune}: status {gst[:16]} want {st[:16]}"
            if not np.array_equal(got, w):
                at = np.nonzero(got != w)[0]
                t = int(np.searchsorted(off, at[0] - GUARD, side="right")) - 1
                raise AssertionError(f"{what} tune={tune} dlead={dlead}: {at.size} bytes differ, first at output byte "
                                     f"{at[0] - GUARD} (slot {t}, which starts at {int(off[max(t, 0)])}): got "
                                     f"{got[at[:8]]}, want {w[at[:8]]}")
    return st[:offs.size - 1], off, w[GUARD:w.size - GUARD]


# ------------------------------------------------------------------ reassembly
def sizes(n, nbytes):
    s = {k: (dt, max(count(n, nbytes), 1)) for k, dt, count in nsx.REASM_FIELDS}
    s["order"] = ("int32", max(n, 1))
    return s


def filled(n, nbytes):
    """Every output and the order at its worst-case size, each byte FILL."""
    out = {}
    for k, (dt, cnt) in sizes(n, nbytes).items():
        size = np.dtype(_NP[dt]).itemsize
        out[k] = torch.full((cnt * size,), FILL, dtype=torch.uint8, device="cuda").view(getattr(torch, dt))
    return out


def to_host(res, n, nbytes):
    return {k: host(res[k]).view(_NP[dt]) for k, (dt, _) in sizes(n, nbytes).items()}


def reasm_gpu(buf, offs, tune=None):
    n = offs.size - 1
    out = filled(n, buf.size)
    order = out.pop("order")
    res = nsx.reasm_ipv4_dev(d(buf), d(offs), out=out, order=order, tune=tune)
    assert all(res[k] is out[k] for k in out) and res["order"] is order
    return to_host(res, n, buf.size)


def reasm_want(buf, offs):
    """The model's outputs laid into FILL-filled arrays of the worst-case sizes: (arrays, the model's dict). With no
    frame, no order is written."""
    n = offs.size - 1
    o = F.reasm(buf, offs)
    w = {}
    for k, (dt, cnt) in sizes(n, buf.size).items():
        size = np.dtype(_NP[dt]).itemsize
        a = np.full(cnt * size, FILL, np.uint8).view(_NP[dt])
        v = np.asarray([o["n_out"]], np.uint64) if k == "n_out" else np.asarray(o[k]).reshape(-1)
        a[:v.size] = v
        w[k] = a
    w["n_super"] = w["n_out"]  # the name tests/_gro_gpu.same reports with
    return w, o


def reasm_same(got, w, what=""):
    got = dict(got, n_super=got["n_out"])
    same(got, w, what)


def reasm_check(buf, offs, tunes=(None,), what=""):
    w, o = reasm_want(buf, offs)
    for tune in tunes:
        reasm_same(reasm_gpu(buf, offs, tune=tune), w, f"{what} tune={tune}")
    return o
