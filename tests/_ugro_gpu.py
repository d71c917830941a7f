"""Shared helpers of the UDP receive-coalescing GPU tests (tests/test_gpu_ugro.py, tests/test_gpu_ugro_fuzz.py), as
tests/_gro_gpu.py is for TCP: one device call of nsx_ugro_* (flow=False) or nsx_ugro_flow_* (flow=True) over outputs
pre-filled with a fill byte, the model's outputs (tests/_ugro.py) laid into arrays filled the same way, their
comparison array for array, and the round trip nsx_udp_rx_*_verify_dev → nsx_ugro_* → nsx_udp_uso_*_build_dev without
leaving the device."""
import numpy as np

import _gro_gpu
import _ugro
from _gpu import host, torch, nsx

FILL = _gro_gpu.FILL
_NP = _gro_gpu._NP
d = _gro_gpu.d
d_valid = _gro_gpu.d_valid


def fn(ipver, flow=False):
    if flow:
        return nsx.ugro_flow_ipv4_dev if ipver == 4 else nsx.ugro_flow_ipv6_dev
    return nsx.ugro_ipv4_dev if ipver == 4 else nsx.ugro_ipv6_dev


def sizes(n, ipver, nbytes, flow=False):
    alen = 4 if ipver == 4 else 16
    s = {k: (dt, max(count(n, alen, nbytes), 1)) for k, dt, count in nsx.UGRO_FIELDS}
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
    o = (_ugro.ugro_flow if flow else _ugro.ugro)(buf, offs, valid, ipver)
    w = {}
    for k, (dt, cnt) in sizes(n, ipver, buf.size, flow).items():
        size = np.dtype(_NP[dt]).itemsize
        a = np.full(cnt * size, FILL, np.uint8).view(_NP[dt])
        v = np.asarray([o["n_super"]], np.uint64) if k == "n_super" else np.asarray(o[k]).reshape(-1)
        a[:v.size] = v
        w[k] = a
    return w, o


same = _gro_gpu.same


def check(buf, offs, valid, ipver, tunes=(None,), what="", flow=False):
    w, o = want(buf, offs, valid, ipver, flow)
    for tune in tunes:
        same(gpu(buf, offs, valid, ipver, tune=tune, flow=flow), w, f"{what} flow={flow} tune={tune}")
    return o


def check_both(buf, offs, valid, ipver, tunes=(None,), what=""):
    return check(buf, offs, valid, ipver, tunes, what), check(buf, offs, valid, ipver, tunes, what, flow=True)


def round_trip(buf, offs, ipver, tune=None, flow=False, keep=None):
    """nsx_udp_rx_*_verify_dev → nsx_ugro_* / nsx_ugro_flow_* → nsx_udp_uso_*_build_dev (flags 0) without leaving the
    device: the mask is the verify's (keep: bits to AND into it), frame_first the prefix sum of frame_cnt, output slots
    the member frames' own lengths padded to a multiple of 4, output position p the input frame p-th among the members
    (with flow: in the order the call returns — the members come first in it). Returns (member frame indices by output
    position, the built frames as a list of bytes): nothing of the numpy model is used."""
    n = offs.size - 1
    d_buf, d_offs = d(buf), d(offs)
    rx = nsx.udp_rx_ipv4_verify_dev if ipver == 4 else nsx.udp_rx_ipv6_verify_dev
    mask = rx(d_buf, d_offs)
    if keep is not None:
        mask &= d_valid(keep, n)
    g = fn(ipver, flow)(d_buf, d_offs, mask, tune=tune)
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
    uso = nsx.udp_uso_ipv4_build_dev if ipver == 4 else nsx.udp_uso_ipv6_build_dev
    uso({k: g[k][:ns * (alen if k in ("src", "dst") else 1)] for k in nsx.IP_FIELDS},
        {k: g[k][:ns] for k in nsx.UDP_FIELDS}, g["data"], g["data_off"][:ns + 1], g["gso"][:ns], frame_first, seg,
        built, out_off)
    z, oo, fl, ps = host(built), host(out_off), host(flen), host(pos)
    return ps, [z[int(oo[p]):int(oo[p]) + int(fl[p])].tobytes() for p in range(nf)]


def assert_round_trip(buf, offs, ipver, tune=None, flow=False, keep=None, members=None, what=""):
    """Every member frame comes back from round_trip byte for byte; members (optional): how many there must be."""
    ps, frames = round_trip(buf, offs, ipver, tune=tune, flow=flow, keep=keep)
    assert members is None or len(ps) == members, f"{what}: {len(ps)} members, {members} expected"
    for p, f in enumerate(ps):
        src = buf[int(offs[f]):int(offs[f + 1])].tobytes()
        assert frames[p] == src, f"{what} flow={flow} tune={tune}: position {p}, frame {f} ({len(src)} B) differs"
    return ps
