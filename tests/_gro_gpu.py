"""Shared helpers of the receive-coalescing GPU tests (tests/test_gpu_gro.py, tests/test_gpu_gro_flow.py and the GRO
family of tests/test_gpu_zz_fuzz.py): one device call of nsx_gro_* (flow=False) or nsx_gro_flow_* (flow=True) over
outputs pre-filled with a fill byte, the model's outputs (tests/_gro.py, tests/_gro_flow.py) laid into arrays filled
the same way, their comparison array for array, and the round trip of a result through nsx_tso_*_build_dev without
leaving the device."""
import numpy as np

import _gro
import _gro_flow
from _gpu import dev, host, torch, nsx, mask_words

FILL = 0xAB
_NP = {"uint8": np.uint8, "int16": np.uint16, "int32": np.uint32, "int64": np.uint64}
_SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
           np.dtype(np.uint64): np.int64}


def d(a):
    a = np.ascontiguousarray(a)
    return dev(a.view(_SIGNED[a.dtype]))


def fn(ipver, flow=False):
    if flow:
        return nsx.gro_flow_ipv4_tcp_dev if ipver == 4 else nsx.gro_flow_ipv6_tcp_dev
    return nsx.gro_ipv4_tcp_dev if ipver == 4 else nsx.gro_ipv6_tcp_dev


def sizes(n, ipver, nbytes, flow=False):
    alen = 4 if ipver == 4 else 16
    s = {k: (dt, max(count(n, alen, nbytes), 1)) for k, dt, count in nsx.GRO_FIELDS}
    if flow:
        s["order"] = ("int32", max(n, 1))
    return s


def filled(n, ipver, nbytes, flow=False):
    """Every output (with flow, the order too) at its worst-case size, each byte FILL."""
    out = {}
    for k, (dt, cnt) in sizes(n, ipver, nbytes, flow).items():
        size = np.dtype(_NP[dt]).itemsize
        out[k] = torch.full((cnt * size,), FILL, dtype=torch.uint8, device="cuda").view(getattr(torch, dt))
    return out


def to_host(res, n, ipver, nbytes, flow=False):
    return {k: host(res[k]).view(_NP[dt]) for k, (dt, _) in sizes(n, ipver, nbytes, flow).items()}


def d_valid(valid, n):
    words = mask_words(_gro.valid_bits(valid, n).astype(np.uint8))
    return d(words if words.size else np.zeros(1, np.uint64))


def gpu(buf, offs, valid, ipver, tune=None, d_mask=None, flow=False):
    """One device call over FILL-filled outputs: dict of host arrays (unsigned views)."""
    n = offs.size - 1
    d_mask = d_valid(valid, n) if d_mask is None else d_mask
    out = filled(n, ipver, buf.size, flow)
    order = out.pop("order", None)
    kw = dict(order=order) if flow else {}
    res = fn(ipver, flow)(d(buf), d(offs), d_mask, out=out, tune=tune, **kw)
    assert all(res[k] is out[k] for k in out) and (not flow or res["order"] is order)
    return to_host(res, n, ipver, buf.size, flow)


def want(buf, offs, valid, ipver, flow=False):
    """The model's outputs laid into FILL-filled arrays of the worst-case sizes: (arrays, the model's dict)."""
    n = offs.size - 1
    o = (_gro_flow.gro_flow if flow else _gro.gro)(buf, offs, valid, ipver)
    w = {}
    for k, (dt, cnt) in sizes(n, ipver, buf.size, flow).items():
        size = np.dtype(_NP[dt]).itemsize
        a = np.full(cnt * size, FILL, np.uint8).view(_NP[dt])
        v = np.asarray([o["n_super"]], np.uint64) if k == "n_super" else np.asarray(o[k]).reshape(-1)
        a[:v.size] = v
        w[k] = a
    return w, o


def same(got, w, what=""):
    for k in ["order"] * ("order" in w) + [k for k in w if k != "order"]:
        if not np.array_equal(got[k], w[k]):
            at = np.nonzero(got[k] != w[k])[0]
            raise AssertionError(f"{what} {k}: {at.size} entries differ, first at {at[0]}: got {got[k][at[:8]]}, "
                                 f"want {w[k][at[:8]]} (n_super got {got['n_super'][0]}, want {w['n_super'][0]})")


def check(buf, offs, valid, ipver, tunes=(None,), what="", flow=False):
    w, o = want(buf, offs, valid, ipver, flow)
    for tune in tunes:
        same(gpu(buf, offs, valid, ipver, tune=tune, flow=flow), w, f"{what} tune={tune}")
    return o


def round_trip(buf, offs, valid, ipver, tune=None, flow=False, d_buf=None, d_offs=None):
    """nsx_gro_* / nsx_gro_flow_* → nsx_tso_*_build_dev without leaving the device: frame_first the prefix sum of
    frame_cnt, output slots the member frames' own lengths padded to a multiple of 4, output position p the input frame
    p-th among the members (with flow: in the order the call returns — the members come first in it). Returns
    (member frame indices by output position, the built frames as a list of bytes): nothing of the numpy model is
    used."""
    n = offs.size - 1
    d_buf = d(buf) if d_buf is None else d_buf
    d_offs = d(offs) if d_offs is None else d_offs
    g = fn(ipver, flow)(d_buf, d_offs, d_valid(valid, n), tune=tune)
    ns = int(g["n_super"].item())
    if ns == 0:
        return np.zeros(0, np.int64), []
    seg_of = g["frame_seg"][:n].to(torch.int64) & 0xFFFFFFFF
    if flow:
        order = g["order"][:n].to(torch.int64) & 0xFFFFFFFF
        nf = int(g["frame_cnt"][:ns].sum().item())
        pos = order[:nf]  # members sort before the non-members (key 0xFFFFFFFF) unless a member has that key too
        assert bool((seg_of[pos] != 0xFFFFFFFF).all()), "a non-member among the first positions of the order"
    else:
        pos = torch.nonzero(seg_of != 0xFFFFFFFF).reshape(-1)
        nf = int(pos.numel())
        assert nf == int(g["frame_cnt"][:ns].sum().item())
    flen = (d_offs[1:] - d_offs[:-1])[pos]
    out_off = torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
    out_off[1:] = torch.cumsum((flen + 3) & ~3, 0)
    frame_first = torch.zeros(ns + 1, dtype=torch.int64, device="cuda")
    frame_first[1:] = torch.cumsum(g["frame_cnt"][:ns].to(torch.int64), 0)
    seg = g["frame_seg"][pos].contiguous()
    alen = 4 if ipver == 4 else 16
    built = torch.full((max(int(out_off[-1].item()), 1),), FILL, dtype=torch.uint8, device="cuda")
    tso = nsx.tso_ipv4_tcp_build_dev if ipver == 4 else nsx.tso_ipv6_tcp_build_dev
    tso({k: g[k][:ns * (alen if k in ("src", "dst") else 1)] for k in nsx.IP_FIELDS},
        {k: g[k][:ns] for k, _ in nsx.BUILD_FIELDS}, g["data"], g["data_off"][:ns + 1], g["mss"][:ns], frame_first, seg,
        built, out_off, opts=g["opts"], opt_off=g["opt_off"][:ns + 1])
    z, oo, fl, ps = host(built), host(out_off), host(flen), host(pos)
    return ps, [z[int(oo[p]):int(oo[p]) + int(fl[p])].tobytes() for p in range(nf)]


def assert_round_trip(buf, offs, valid, ipver, untouched=None, tune=None, flow=False, what=""):
    """Every member frame (of those `untouched` marks, default all) comes back from round_trip byte for byte."""
    ps, frames = round_trip(buf, offs, valid, ipver, tune=tune, flow=flow)
    for p, f in enumerate(ps):
        if untouched is None or untouched[f]:
            src = buf[int(offs[f]):int(offs[f + 1])].tobytes()
            assert frames[p] == src, f"{what} flow={flow} tune={tune}: position {p}, frame {f} ({len(src)} B) differs"
    return ps
