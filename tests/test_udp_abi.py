"""The UDP passes' boundary (nsx_udp_*), on any host: the symbols, every NSX_EINVAL before NSX_ENODEV, the two layout
helpers against the restatement tests/_udp.py, the binding's extent checks, and that restatement held to what already
exists — nsx.csum16 over pseudo-header ‖ datagram, the oracle's IPv4 header checksum, and its own receive side over its
own transmit side. The GPU tests (tests/test_gpu_udp.py, tests/test_gpu_udp_fuzz.py) compare the kernels against
tests/_udp.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nsx
import _tso
import _udp
from oracle import csum_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX_CALLS = ("nsx_udp_tx_ipv4_build_dev", "nsx_udp_tx_ipv6_build_dev")
USO_CALLS = ("nsx_udp_uso_ipv4_build_dev", "nsx_udp_uso_ipv6_build_dev")
RX_CALLS = ("nsx_udp_rx_ipv4_verify_dev", "nsx_udp_rx_ipv6_verify_dev")
DEV_CALLS = TX_CALLS + USO_CALLS + RX_CALLS
HOST_CALLS = ("nsx_udp_layout_host", "nsx_udp_uso_layout_host")
fake = ctypes.c_void_p(0x1000)
E, D = nsx.NSX_EINVAL, nsx.NSX_ENODEV


# ---------------------------------------------------------------- symbols
def test_udp_symbols_are_declared_and_exported(tmp_path):
    """nsx_csum.h declares exactly the eight calls and nsx_udp_tune.h exactly the six _tuned twins of the device
    calls; nsx_tune.h and the other tune headers name none of them; the library exports them all; the ABI version
    stays 2; a plain C caller compiles against both headers and gets the documented codes."""
    inc = os.path.join(ROOT, "include")
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)  # noqa: E731
    decl = r"^int\s+(nsx_udp_[a-z_0-9]+)\("
    text = open(os.path.join(inc, "nsx_csum.h")).read()
    assert set(re.findall(decl, strip(text), flags=re.M)) == set(DEV_CALLS) | set(HOST_CALLS)
    tune = open(os.path.join(inc, "nsx_udp_tune.h")).read()
    assert set(re.findall(decl, strip(tune), flags=re.M)) == {c + "_tuned" for c in DEV_CALLS}
    assert '#include "nsx_tune.h"' in tune
    for h in ("nsx_tune.h", "nsx_tx_tune.h", "nsx_gro_tune.h"):
        assert "nsx_udp_" not in strip(open(os.path.join(inc, h)).read()), h
    out = subprocess.run(["nm", "-D", "--defined-only", nsx.LIB_PATH], capture_output=True, text=True).stdout
    exported = {s for s in re.findall(r" T (nsx_\w+)", out) if s.startswith("nsx_udp_")}
    assert exported == set(DEV_CALLS) | set(HOST_CALLS) | {c + "_tuned" for c in DEV_CALLS}
    assert nsx.abi_version() == 2
    assert "NSX_ABI_VERSION 2 " in text
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for word in ("a computed checksum of 0 is sent as 0xFFFF", "a received field of 0 means \"no checksum\" on IPv4",
                 "a received field of 0 is illegal on IPv6", "nsx_tso_count_host(h_data_off, h_gso, n, h_frame_first) "
                 "is used as it stands", "__udp_gso_segment", "8 <= U <= P", "can be captured into a graph",
                 "A built frame's raw is never 0", "65507 bytes (IPv4) or 65527 bytes (IPv6)"):
        assert word in flat, word
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include "nsx_csum.h"
#include "nsx_udp_tune.h"
int main(void) {
    uint64_t doff[3] = {0, 5, 1477}, out[3] = {0}, first[3] = {0, 1, 2}, bad[3] = {0, 1, 3};
    uint32_t gso[2] = {1472, 1472}, seg[2] = {9, 9};
    nsx_ip_hdr_soa ip = {0};
    nsx_udp_hdr_soa udp = {0};
    nsx_tune t = {0};
    if (nsx_udp_layout_host(doff, 2, 20, out) != NSX_OK || out[1] != 36 || out[2] != 36 + 1500) return 1;
    if (nsx_udp_layout_host(doff, 2, 40, out) != NSX_OK || out[1] != 56 || out[2] != 56 + 1520) return 2;
    if (nsx_udp_layout_host(doff, 2, 24, out) != NSX_EINVAL) return 3;
    if (nsx_udp_uso_layout_host(doff, gso, first, 2, 20, seg, out) != NSX_OK || seg[0] != 0 || seg[1] != 1) return 4;
    if (nsx_udp_uso_layout_host(doff, gso, bad, 2, 20, seg, out) != NSX_EINVAL) return 5;
    if (nsx_udp_tx_ipv4_build_dev(&ip, &udp, 0, doff, 0, 2, 0, (uint8_t*)out, out, 0, 0) != NSX_EINVAL) return 6;
    if (nsx_udp_tx_ipv6_build_dev_tuned(&ip, &udp, 0, doff, 0, 0, NSX_UDP_NO_CSUM, 0, 0, 0, 0, &t) != NSX_EINVAL) return 7;
    if (nsx_udp_rx_ipv4_verify_dev(0, doff, 2, out, 0, 0, 0) != NSX_EINVAL) return 8;
    if (nsx_udp_rx_ipv6_verify_dev_tuned(0, 0, 0, 0, 0, 0, &t) != NSX_OK) return 9;
    return 0;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(nsx.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I", inc, "-L", libdir, "-lnsx_csum",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- validation
def _soas(ip_kw=None, udp_kw=None):
    ip = nsx.IpHdrSoA(src=0x1000, dst=0x1000)
    udp = nsx.UdpHdrSoA(src_port=0x1000, dst_port=0x1000)
    for k, v in (ip_kw or {}).items():
        setattr(ip, k, v)
    for k, v in (udp_kw or {}).items():
        setattr(udp, k, v)
    return ip, udp


def _tx(name, tuned=False, **kw):
    a = dict(ip={}, udp={}, ipp=True, udpp=True, data=fake, data_off=fake, data_bytes=100, n=10, flags=0, out=fake,
             out_off=fake, raw=fake)
    a.update(kw)
    ip, udp = _soas(a["ip"], a["udp"])
    args = [ctypes.byref(ip) if a["ipp"] else None, ctypes.byref(udp) if a["udpp"] else None, a["data"],
            a["data_off"], a["data_bytes"], a["n"], a["flags"], a["out"], a["out_off"], a["raw"], None]
    fn = getattr(nsx.lib(), name + ("_tuned" if tuned else ""))
    return fn(*(args + [None] if tuned else args))


def _uso(name, tuned=False, **kw):
    a = dict(ip={}, udp={}, ipp=True, udpp=True, data=fake, data_off=fake, data_bytes=100, gso=fake, n=10, first=fake,
             seg=fake, nf=20, flags=0, out=fake, out_off=fake, raw=fake)
    a.update(kw)
    ip, udp = _soas(a["ip"], a["udp"])
    args = [ctypes.byref(ip) if a["ipp"] else None, ctypes.byref(udp) if a["udpp"] else None, a["data"],
            a["data_off"], a["data_bytes"], a["gso"], a["n"], a["first"], a["seg"], a["nf"], a["flags"], a["out"],
            a["out_off"], a["raw"], None]
    fn = getattr(nsx.lib(), name + ("_tuned" if tuned else ""))
    return fn(*(args + [None] if tuned else args))


_BUILD_BAD = (dict(ipp=False), dict(udpp=False), dict(ip=dict(src=None)), dict(ip=dict(dst=None)),
              dict(udp=dict(src_port=None)), dict(udp=dict(dst_port=None)), dict(data_off=None), dict(out=None),
              dict(out_off=None), dict(data=None), dict(flags=2), dict(flags=0x80000000), dict(flags=3))


@pytest.mark.parametrize("tuned", [False, True], ids=["plain", "tuned"])
def test_udp_build_calls_validate_before_any_device_work(tuned):
    """NULL structs, NULL required members, NULL arrays, d_data NULL with data_bytes nonzero, unknown flag bits and
    NO_CSUM on IPv6 are NSX_EINVAL before anything else; a bad flag even with n == 0. A well-formed call on a host
    with no GPU is NSX_ENODEV; n == 0 is NSX_OK without a device. The optional members (ident, ttl, tclass, flow),
    d_udp_raw and d_data with data_bytes == 0 may be NULL."""
    for name in TX_CALLS:
        v6 = "ipv6" in name
        for kw in _BUILD_BAD:
            assert _tx(name, tuned, **kw) == E, (name, kw)
        if v6:
            assert _tx(name, tuned, flags=1) == E and _tx(name, tuned, flags=1, n=0) == E
        assert _tx(name, tuned, flags=2, n=0) == E
        assert _tx(name, tuned, n=0) == nsx.NSX_OK
        assert _tx(name, tuned, n=0, ipp=False, udpp=False, data_off=None, out=None, out_off=None) == nsx.NSX_OK
        if nsx.device_count() == 0:
            assert _tx(name, tuned) == D
            assert _tx(name, tuned, raw=None) == D and _tx(name, tuned, data=None, data_bytes=0) == D
            if not v6:
                assert _tx(name, tuned, flags=1) == D
    for name in USO_CALLS:
        v6 = "ipv6" in name
        for kw in _BUILD_BAD + (dict(gso=None), dict(first=None), dict(seg=None), dict(n=0), dict(n=1 << 32),
                                dict(n=21), dict(n=10, nf=9)):
            assert _uso(name, tuned, **kw) == E, (name, kw)
        if v6:
            assert _uso(name, tuned, flags=1) == E and _uso(name, tuned, flags=1, nf=0) == E
        assert _uso(name, tuned, nf=0) == nsx.NSX_OK and _uso(name, tuned, nf=0, n=0, gso=None) == nsx.NSX_OK
        if nsx.device_count() == 0:
            assert _uso(name, tuned) == D and _uso(name, tuned, raw=None) == D and _uso(name, tuned, n=20) == D
            if not v6:
                assert _uso(name, tuned, flags=1) == D


def test_udp_rx_calls_validate_before_any_device_work():
    L = nsx.lib()
    for v in (4, 6):
        extra = (fake,) if v == 4 else ()  # d_ip_raw
        for tuned in (False, True):
            fn = getattr(L, f"nsx_udp_rx_ipv{v}_verify_dev" + ("_tuned" if tuned else ""))
            tail = (None, None) if tuned else (None,)
            call = lambda base, offs, n, mask, raw=fake: fn(base, offs, n, mask, *extra, raw, *tail)  # noqa: E731
            assert call(None, fake, 5, fake) == E and call(fake, None, 5, fake) == E and call(fake, fake, 5, None) == E
            assert call(fake, fake, (1 << 40) + 1, fake) == E
            assert call(None, None, 0, None) == nsx.NSX_OK
            if nsx.device_count() == 0:
                assert call(fake, fake, 5, fake) == D and call(fake, fake, 5, fake, None) == D


# ---------------------------------------------------------------- the layout helpers
def test_udp_layout_host_against_the_model():
    rng = np.random.default_rng(0x0D91)
    for ipver in (4, 6):
        for n in (0, 1, 2, 77):
            lens = rng.integers(0, 3000, n)
            c = _udp.Case(rng, ipver, lens, lead=int(rng.integers(4)))
            got = nsx.udp_layout_host(c.data_off, _udp.IPH[ipver])
            assert np.array_equal(got, c.packed())
            assert not (got & np.uint64(3)).any()
            assert np.array_equal(np.diff(got), (c.flen + np.uint64(3)) & ~np.uint64(3))
    L = nsx.lib()
    doff = np.array([0, 10, 5, 20], np.uint64)
    out = np.full(4, 77, np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert L.nsx_udp_layout_host(p(doff), 3, 20, p(out)) == E and (out == 77).all()  # decreasing: nothing written
    ok = np.array([0, 10, 15, 20], np.uint64)
    for iph in (0, 24, 28, 48, 60):
        assert L.nsx_udp_layout_host(p(ok), 3, iph, p(out)) == E
    assert L.nsx_udp_layout_host(None, 3, 20, p(out)) == E and L.nsx_udp_layout_host(p(ok), 3, 20, None) == E
    assert L.nsx_udp_layout_host(None, 0, 20, p(out)) == nsx.NSX_OK and out[0] == 0
    assert (out[1:] == 77).all()


def test_udp_uso_layout_host_against_the_model():
    """The frame map is nsx_tso_count_host's as it stands; frame_seg and the packed offsets against the model; every
    NSX_EINVAL of nsx_tso_layout_host, with nothing written."""
    rng = np.random.default_rng(0x0D92)
    for ipver in (4, 6):
        for gso in (1, 7, 512, 1472):
            lens = [0, 1, max(gso - 1, 0), gso, gso + 1, 3 * gso - 1, 3 * gso, 3 * gso + 1]
            b = _udp.Batch(rng, ipver, lens, gso, lead=1)
            first = nsx.tso_count_host(b.sup.data_off, b.gso)
            assert np.array_equal(first, b.first)
            seg, off = nsx.udp_uso_layout_host(b.sup.data_off, b.gso, first, _udp.IPH[ipver])
            assert np.array_equal(seg, b.seg) and np.array_equal(off, b.off)
            c = _udp.expand(b)
            assert np.array_equal(off, c.packed()) and c.n == b.nf
            assert np.array_equal(np.diff(b.first), [1, 1, 1, 1, 2, 3 if gso > 1 else 2, 3, 4])
    b = _udp.Batch(rng, 4, [100, 0, 3000], [7, 9, 1472])
    L = nsx.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    seg, off = np.full(b.nf, 77, np.uint32), np.full(b.nf + 1, 77, np.uint64)

    def call(doff=b.sup.data_off, gso=b.gso, first=b.first, n=b.n, iph=20, s=seg, o=off):
        return L.nsx_udp_uso_layout_host(p(doff), p(gso), p(first), n, iph, p(s), p(o))

    assert call() == nsx.NSX_OK and np.array_equal(seg, b.seg) and np.array_equal(off, b.off)
    seg[:], off[:] = 77, 77
    zero = b.gso.copy()
    zero[1] = 0
    dec = b.sup.data_off.copy()
    dec[1], dec[2] = dec[2] + np.uint64(1), dec[1]
    lie = b.first.copy()
    lie[1] += np.uint64(1)
    short = b.first.copy()
    short[-1] -= np.uint64(1)
    for kw in (dict(gso=zero), dict(doff=dec), dict(first=lie), dict(first=short), dict(iph=24), dict(iph=0),
               dict(doff=None), dict(gso=None), dict(first=None), dict(o=None), dict(s=None), dict(n=1 << 32)):
        assert call(**kw) == E, kw
        assert (seg == 77).all() and (off == 77).all(), kw
    with pytest.raises(nsx.NsxError):
        nsx.udp_uso_layout_host(b.sup.data_off, zero, b.first)


# ---------------------------------------------------------------- the binding's extent checks
def test_udp_binding_checks_extents_before_the_c_call():
    """Every tensor is checked before the C call (CPU tensors here: a well-formed call is then refused as not on a
    device)."""
    import torch
    n = 10
    i64 = lambda k: torch.zeros(k, dtype=torch.int64)  # noqa: E731
    i16 = lambda k: torch.zeros(k, dtype=torch.int16)  # noqa: E731
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8)  # noqa: E731
    for ipver in (4, 6):
        alen, fmin = (4, 28) if ipver == 4 else (16, 48)
        fn = nsx.udp_tx_ipv4_build_dev if ipver == 4 else nsx.udp_tx_ipv6_build_dev
        base = dict(ip=dict(src=u8(alen * n), dst=u8(alen * n), ident=i16(n), ttl=u8(n)),
                    ports=dict(src_port=i16(n), dst_port=i16(n)), data=u8(100), data_off=i64(n + 1),
                    out=u8(fmin * n), out_off=i64(n + 1), raw=i16(n))
        cases = [(dict(ip=dict(base["ip"], src=None)), "'src' missing"), (dict(ip=dict(base["ip"], dst=u8(alen * n - 1))), " dst"),
                 (dict(ip=dict(base["ip"], ident=u8(2 * n))), "2-byte elements"),
                 (dict(ip=dict(base["ip"], ttl=u8(n - 1))), " ttl"),
                 (dict(ports=dict(src_port=i16(n))), "'dst_port' missing"),
                 (dict(ports=dict(src_port=i16(n - 1), dst_port=i16(n))), " src_port"),
                 (dict(ports=dict(src_port=u8(2 * n), dst_port=i16(n))), "2-byte elements"),
                 (dict(out_off=i64(n)), " out_off"), (dict(out=u8(fmin * n - 1)), " out"),
                 (dict(out=i16(fmin * n)), "1-byte elements"), (dict(raw=i16(n - 1)), " raw"),
                 (dict(data_off=torch.zeros(n + 1, dtype=torch.int32)), "8-byte elements"),
                 (dict(data=u8(200)[::2]), "contiguous"), (dict(), "device")]
        for kw, msg in cases:
            with pytest.raises(ValueError) as e:
                fn(**dict(base, **kw))
            assert msg in str(e.value), (msg, str(e.value))
        nf = 25
        fn = nsx.udp_uso_ipv4_build_dev if ipver == 4 else nsx.udp_uso_ipv6_build_dev
        base = dict(base, gso=torch.zeros(n, dtype=torch.int32), frame_first=i64(n + 1),
                    frame_seg=torch.zeros(nf, dtype=torch.int32), out=u8(fmin * nf), out_off=i64(nf + 1), raw=i16(nf))
        cases = [(dict(gso=torch.zeros(n - 1, dtype=torch.int32)), " gso"), (dict(gso=i64(n)), "4-byte elements"),
                 (dict(frame_first=i64(n)), " frame_first"), (dict(frame_seg=torch.zeros(nf - 1, dtype=torch.int32)), " frame_seg"),
                 (dict(raw=i16(nf - 1)), " raw"), (dict(out=u8(fmin * nf - 1)), " out"),
                 (dict(n_frames=5), "5 frames for 10"), (dict(n_frames=-1), "n_frames"),
                 (dict(ports=dict(src_port=i16(n))), "'dst_port' missing"), (dict(), "device")]
        for kw, msg in cases:
            with pytest.raises(ValueError) as e:
                fn(**dict(base, **kw))
            assert msg in str(e.value), (msg, str(e.value))
        fn = nsx.udp_rx_ipv4_verify_dev if ipver == 4 else nsx.udp_rx_ipv6_verify_dev
        n = 70
        base = dict(buf=u8(100), offsets=i64(n + 1), mask=i64(2), udp_raw=i16(n))
        cases = [(dict(mask=i64(1)), " mask"), (dict(mask=torch.zeros(4, dtype=torch.int32)), "8-byte elements"),
                 (dict(udp_raw=i16(n - 1)), " udp_raw"), (dict(offsets=torch.zeros(n + 1, dtype=torch.int32)), "8-byte"),
                 (dict(), "device")]
        if ipver == 4:
            cases.insert(0, (dict(ip_raw=i16(n - 1)), " ip_raw"))
        for kw, msg in cases:
            with pytest.raises(ValueError) as e:
                fn(**dict(base, **kw))
            assert msg in str(e.value), (msg, str(e.value))
        n = 10


# ---------------------------------------------------------------- the model, held to what exists
def _model_case(ipver):
    rng = np.random.default_rng(0x0D93 + ipver)
    lens = [0, 1, 2, 3, 4, 7, 8, 15, 16, 17, 995, 996, 997, 1472, 2019, 2020, 2021, 33, 34, 9000]
    c = _udp.Case(rng, ipver, lens, lead=3)
    _udp.craft_ffff(c, 17, 10)
    _udp.craft_ffff(c, 18, 11)
    return c


@pytest.mark.parametrize("ipver", [4, 6])
def test_model_frames_verify_under_csum16_and_the_oracle(ipver):
    """For every expected frame nsx.csum16(pseudo, datagram) is 0xFFFF, and its field-zero sum is the reported raw;
    the IPv4 header verifies under the oracle's checksum; crafted frames carry the field 0xFFFF, never 0x0000; the
    frame's fields sit where RFC 768 / 791 / 8200 put them."""
    c = _model_case(ipver)
    h = _udp.IPH[ipver]
    fr, raws = _udp.frames(c)
    for i, f in enumerate(fr):
        d = f[h:]
        ps = _udp.pseudo(ipver, c.ip["src"][i], c.ip["dst"][i], d.size)
        assert nsx.csum16(ps.tobytes(), d.tobytes()) == 0xFFFF, i
        z = d.copy()
        z[6:8] = 0
        assert nsx.csum16(ps.tobytes(), z.tobytes()) == raws[i] == O.c_go_checksum(ps.tobytes(), z.tobytes())
        assert (int(d[6]) << 8 | int(d[7])) != 0
        assert (int(d[4]) << 8 | int(d[5])) == d.size == 8 + int(c.plen[i])
        assert (int(d[0]) << 8 | int(d[1])) == c.ports["src_port"][i]
        assert (int(d[2]) << 8 | int(d[3])) == c.ports["dst_port"][i]
        if ipver == 4:
            assert O.c_go_checksum(b"", f[:20].tobytes()) == 0xFFFF
            assert f[0] == 0x45 and f[9] == 17 and (int(f[2]) << 8 | int(f[3])) == f.size and f[6] == 0x40
            assert bytes(f[12:16]) == bytes(c.ip["src"][i]) and bytes(f[16:20]) == bytes(c.ip["dst"][i])
        else:
            assert f[0] >> 4 == 6 and f[6] == 17 and (int(f[4]) << 8 | int(f[5])) == d.size
            assert bytes(f[8:24]) == bytes(c.ip["src"][i]) and bytes(f[24:40]) == bytes(c.ip["dst"][i])
    for i in (17, 18):
        assert raws[i] == 0xFFFF and bytes(fr[i][h + 6:h + 8]) == b"\xff\xff"
    if ipver == 4:
        nc, nraws = _udp.frames(c, flags=_udp.NO_CSUM)
        assert np.array_equal(nraws, raws) and all(bytes(f[26:28]) == b"\0\0" for f in nc)
    dflt, _ = _udp.frames(c, null=("ident", "ttl", "tclass", "flow"))
    if ipver == 4:
        assert all(f[8] == 64 and f[4] == 0 and f[5] == 0 for f in dflt)
    else:
        assert all(f[7] == 64 and bytes(f[:4]) == b"\x60\0\0\0" for f in dflt)


@pytest.mark.parametrize("ipver", [4, 6])
def test_model_receive_side_accepts_the_model_transmit_side(ipver):
    """Every built frame is valid under rx_expected — with NO_CSUM too on IPv4 — and a frame past the length limit is
    not built; the edge batch's verdicts are the ones its names say."""
    c = _model_case(ipver)
    fr, _ = _udp.frames(c)
    buf, offs = _udp.concat(fr, lead=1)
    valid, ipr, udr = _udp.rx_expected(ipver, buf, offs)
    assert valid.all() and (udr == 0xFFFF).all() and (ipver == 6 or (ipr == 0xFFFF).all())
    if ipver == 4:
        nc, raws = _udp.frames(c, flags=_udp.NO_CSUM)
        valid, _, udr = _udp.rx_expected(4, *_udp.concat(nc))
        assert valid.all() and np.array_equal(udr, raws)
    big = _udp.Case(np.random.default_rng(1), ipver, [_udp.PAY_MAX[ipver], _udp.PAY_MAX[ipver] + 1])
    fr, raws = _udp.frames(big)
    assert fr[0] is not None and fr[1] is None and raws[0] != 0 and raws[1] == 0
    want_valid = {"field_ffff_crafted", "u_eq_p", "u_lt_p_junk_padding", "ihl6_options", "len_28", "len_48", "frame_64k"}
    edge = _udp.rx_edge_frames(ipver)
    valid, ipr, udr = _udp.rx_expected(ipver, *_udp.concat([f for _, f in edge], lead=1))
    for (name, f), v, r in zip(edge, valid, udr):
        want = name.startswith("valid_") or name in want_valid or (ipver == 4 and name.startswith("field_zero"))
        assert v == want, (name, v, hex(r))
    assert len({name for name, _ in edge}) == len(edge)


@pytest.mark.parametrize("ipver", [4, 6])
def test_model_uso_expansion(ipver):
    """The expanded batch: slices tile each super-datagram's payload, ident counts up modulo 2^16, everything else is
    copied; a lying frame_seg entry yields a slice inside the super-datagram it names."""
    rng = np.random.default_rng(0x0D94 + ipver)
    b = _udp.Batch(rng, ipver, [0, 1, 20, 21, 22, 100], 7, lead=2)
    b.sup.ip["ident"][5] = 0xFFFA
    c = _udp.expand(b)
    seg, j = _tso.frame_index(b.first)
    assert c.data_off is not None and np.array_equal(c.plen, [0, 1, 7, 7, 6, 7, 7, 7, 7, 7, 7, 1] + [7] * 14 + [2])
    assert np.array_equal(c.ip["ident"], (b.sup.ip["ident"][seg].astype(np.int64) + j) & 0xFFFF)
    assert 0 in c.ip["ident"][seg == 5].tolist()  # the wrap
    for k in ("src_port", "dst_port"):
        assert np.array_equal(c.ports[k], b.sup.ports[k][seg])
    lie = b.seg.copy()
    lie[3] = 5  # frame 3 (of super-datagram 2) claims super-datagram 5: j = 3 - first[5] wraps, the slice is empty
    cl = _udp.expand(b, seg=lie)
    assert cl.data_off is None and cl.plen[3] == 0 and cl.lo[3] == b.sup.data_off[6]
    lie[3] = 1  # j = 3 - 1 = 2 in a 1-byte super-datagram: empty, at its end
    cl = _udp.expand(b, seg=lie)
    assert cl.plen[3] == 0 and cl.lo[3] == b.sup.data_off[2]
    fr, _ = _udp.frames(c)
    valid, _, _ = _udp.rx_expected(ipver, *_udp.concat(fr))
    assert valid.all()
