"""The fused transmit pass's boundary (nsx_tx_*), on any host: validation before any device work, the layout
call, the binding's extent checks, and the self-checks of the expected-frame helper tests/_tx.py that the GPU tests
(tests/test_gpu_tx.py) compare against."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nsx
import _tx
from oracle import csum_oracle as O

DEV_CALLS = ("nsx_tx_ipv4_tcp_build_dev", "nsx_tx_ipv6_tcp_build_dev")
HOST_CALLS = ("nsx_tx_ipv4_tcp_build_host", "nsx_tx_ipv6_tcp_build_host")
fake = ctypes.c_void_p(0x1000)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tx_symbols_are_declared_and_exported(tmp_path):
    """The boundary header declares the five tx calls, nsx_tx_tune.h (part of nsx_tune.h) their four _tuned twins;
    the library exports all nine; NSX_ABI_VERSION stays 2 (symbols were only added); and a plain C caller that
    includes nsx_tune.h alone compiles against them and gets NSX_EINVAL / 0 from the validation."""
    inc = os.path.join(ROOT, "include")
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, p)).read(), flags=re.S)  # noqa: E731
    plain = set(re.findall(r"^int (nsx_tx_[a-z_0-9]+)\(", strip("nsx_csum.h"), flags=re.M))
    tuned = set(re.findall(r"^int (nsx_tx_[a-z_0-9]+)\(", strip("nsx_tx_tune.h"), flags=re.M))
    assert plain == set(DEV_CALLS) | set(HOST_CALLS) | {"nsx_tx_layout_host"}
    assert tuned == {f + "_tuned" for f in DEV_CALLS + HOST_CALLS}
    assert '#include "nsx_tx_tune.h"' in open(os.path.join(inc, "nsx_tune.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", nsx.LIB_PATH], capture_output=True, text=True).stdout
    assert plain | tuned <= set(re.findall(r" T (nsx_\w+)", out))
    assert nsx.abi_version() == 2
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include "nsx_tune.h"
int main(void) {
    nsx_ip_hdr_soa ip = {0};
    nsx_tcp_hdr_soa tcp = {0};
    nsx_tune t = {0};
    uint64_t off[1] = {7};
    if (nsx_tx_ipv4_tcp_build_dev_tuned(&ip, &tcp, 0, 0, 0, off, 0, 1, 0, off, 0, 0, &t) != NSX_EINVAL) return 1;
    if (nsx_tx_ipv6_tcp_build_host_tuned(&ip, &tcp, 0, 0, 0, off, 1, 0, off, 0, 0, &t) != NSX_EINVAL) return 2;
    if (nsx_tx_ipv6_tcp_build_dev(&ip, &tcp, 0, 0, 0, off, 0, 0, 0, off, 0, 0) != NSX_OK) return 3;
    if (nsx_tx_layout_host(0, 0, 0, 40, off) != NSX_OK || off[0] != 0) return 4;
    return nsx_tx_layout_host(0, 0, 0, 24, off) == NSX_EINVAL ? 0 : 5;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(nsx.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I", inc, "-L", libdir, "-lnsx_csum",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def _soas(ip_null=(), tcp_null=()):
    ip = nsx.IpHdrSoA(*[None if k in ip_null else 0x1000 for k in nsx.IP_FIELDS])
    tcp = nsx.TcpHdrSoA(*[None if k in tcp_null else 0x1000 for k, _ in nsx.BUILD_FIELDS])
    return ip, tcp


def _dev_call(name, ip, tcp, n=4, tuned=False, **kw):
    """One raw device call with fake pointers (validation must refuse or pass it before any device work)."""
    a = dict(opts=None, opt_off=None, data=fake, data_off=fake, data_bytes=64, out=fake, out_off=fake, raw=None)
    a.update(kw)
    args = [None if ip is None else ctypes.byref(ip), None if tcp is None else ctypes.byref(tcp), a["opts"],
            a["opt_off"], a["data"], a["data_off"], a["data_bytes"], n, a["out"], a["out_off"], a["raw"], None]
    if tuned:
        return getattr(nsx.lib(), name + "_tuned")(*args, ctypes.byref(nsx.Tune(run_segs=16)))
    return getattr(nsx.lib(), name)(*args)


def test_tx_device_calls_validate_before_any_device_work():
    """n == 0 is a no-op; NULL ip, ip->src, ip->dst, tcp or a required TCP field, a NULL out / offsets array, or
    opt_off without opts is NSX_EINVAL; the optional ident / ttl / tclass / flow / offset may be NULL; and with no
    GPU every device entry point and every _tuned twin then answers NSX_ENODEV."""
    ip, tcp = _soas()
    for name in DEV_CALLS:
        for tuned in (False, True):
            assert _dev_call(name, None, None, n=0, tuned=tuned) == 0
            assert _dev_call(name, None, tcp, tuned=tuned) == nsx.NSX_EINVAL
            assert _dev_call(name, ip, None, tuned=tuned) == nsx.NSX_EINVAL
            for k in ("src", "dst"):
                assert _dev_call(name, _soas(ip_null=(k,))[0], tcp, tuned=tuned) == nsx.NSX_EINVAL, k
            for k, _ in nsx.BUILD_FIELDS:
                if k != "offset":
                    assert _dev_call(name, ip, _soas(tcp_null=(k,))[1], tuned=tuned) == nsx.NSX_EINVAL, k
            for kw in (dict(out=None), dict(out_off=None), dict(data_off=None), dict(data=None),
                       dict(opt_off=fake, opts=None)):
                assert _dev_call(name, ip, tcp, tuned=tuned, **kw) == nsx.NSX_EINVAL, kw
            if nsx.device_count() == 0:
                assert _dev_call(name, ip, tcp, tuned=tuned) == nsx.NSX_ENODEV
                opt = _soas(ip_null=("ident", "ttl", "tclass", "flow"), tcp_null=("offset",))
                assert _dev_call(name, *opt, tuned=tuned) == nsx.NSX_ENODEV


def _host_case(ipver, n=3, pay=10):
    rng = np.random.default_rng(ipver)
    return _tx.Case(rng, ipver, [pay] * n)


def test_tx_host_calls_validate_before_any_device():
    """The host calls check every span before touching a device: a well-formed batch is NSX_ENODEV on a GPU-less
    host, a malformed one NSX_EINVAL everywhere — a missing address array or TCP field, slots that are not 4-aligned
    or too short for frame + padding, decreasing offsets; n == 0 returns 0."""
    for ipver, name in zip((4, 6), HOST_CALLS):
        fn = getattr(nsx, f"tx_ipv{ipver}_tcp_build_host")
        c = _host_case(ipver)
        if nsx.device_count() == 0:
            for tune in (None, dict(shards_per_device=3)):
                with pytest.raises(nsx.NsxError) as e:
                    fn(c.ip, c.fields, c.data, c.data_off, tune=tune)
                assert e.value.code == nsx.NSX_ENODEV
        lay = c.packed()
        total = int(lay[-1])
        slot = int(lay[1])
        bad_layouts = [lay + np.uint64(2), np.array([0, slot, 2 * slot - 4, 3 * slot], np.uint64),
                       np.array([0, slot, 2 * slot, 2 * slot], np.uint64)]
        for oo in bad_layouts:
            with pytest.raises(nsx.NsxError) as e:
                fn(c.ip, c.fields, c.data, c.data_off, out_off=oo, out=np.zeros(total + 8, np.uint8))
            assert e.value.code == nsx.NSX_EINVAL, oo
        with pytest.raises(nsx.NsxError) as e:
            fn(c.ip, c.fields, c.data, np.array([0, 10, 5, 30], np.uint64), out_off=lay, out=np.zeros(total, np.uint8))
        assert e.value.code == nsx.NSX_EINVAL
        # raw C calls: NULL structs and members, n == 0
        L = nsx.lib()
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        out = np.zeros(total, np.uint8)

        def call(ip, tcp, n=3, tuned=False):
            args = [None if ip is None else ctypes.byref(ip), None if tcp is None else ctypes.byref(tcp), None, None,
                    ptr(c.data), ptr(c.data_off), n, ptr(out), ptr(lay), None, 0]
            return getattr(L, name + "_tuned")(*args, None) if tuned else getattr(L, name)(*args)

        def soas(ip_null=(), tcp_null=()):
            return (nsx.IpHdrSoA(*[None if k in ip_null else c.ip[k].ctypes.data for k in nsx.IP_FIELDS]),
                    nsx.TcpHdrSoA(*[None if k in tcp_null else c.fields[k].ctypes.data for k, _ in nsx.BUILD_FIELDS]))

        ip, tcp = soas()
        for tuned in (False, True):
            assert call(None, None, n=0, tuned=tuned) == 0
            assert call(None, tcp, tuned=tuned) == nsx.NSX_EINVAL
            assert call(ip, None, tuned=tuned) == nsx.NSX_EINVAL
            assert call(soas(ip_null=("src",))[0], tcp, tuned=tuned) == nsx.NSX_EINVAL
            assert call(soas(ip_null=("dst",))[0], tcp, tuned=tuned) == nsx.NSX_EINVAL
            assert call(ip, soas(tcp_null=("window",))[1], tuned=tuned) == nsx.NSX_EINVAL


@pytest.mark.parametrize("ipver", [4, 6])
def test_tx_host_calls_refuse_a_frame_that_does_not_fit_its_length_field(ipver):
    """A frame whose TCP part exceeds the IP length field (IPv4 wire 65516, IPv6 wire 65536) makes the host call
    NSX_EINVAL before any device is touched; one byte shorter (65515 / 65535) passes validation — NSX_ENODEV on a
    GPU-less host, built otherwise."""
    fn = getattr(nsx, f"tx_ipv{ipver}_tcp_build_host")
    top = _tx.WIRE_MAX[ipver]
    rng = np.random.default_rng(0x70 + ipver)
    over = _tx.Case(rng, ipver, [10, top + 1 - 20, 10])
    assert int(over.wire[1]) == top + 1
    with pytest.raises(nsx.NsxError) as e:
        fn(over.ip, over.fields, over.data, over.data_off)
    assert e.value.code == nsx.NSX_EINVAL
    fits = _tx.Case(rng, ipver, [10, top - 20, 10])
    assert int(fits.wire[1]) == top
    if nsx.device_count() == 0:
        with pytest.raises(nsx.NsxError) as e:
            fn(fits.ip, fits.fields, fits.data, fits.data_off)
        assert e.value.code == nsx.NSX_ENODEV
    else:
        got, raw = fn(fits.ip, fits.fields, fits.data, fits.data_off)
        want, wraw = _tx.expected(fits, fits.packed())
        assert np.array_equal(got, want) and np.array_equal(raw, wraw)
    # with options: the option bytes and their padding count
    ob = [b"", _tx.opt_bytes(rng, "nop"), b""]  # 1 option byte + 1 pad: a 22-byte header
    over = _tx.Case(rng, ipver, [10, top + 1 - 22, 10], opts=ob)
    assert int(over.wire[1]) == top + 1
    with pytest.raises(nsx.NsxError) as e:
        fn(over.ip, over.fields, over.data, over.data_off, opts=over.opts, opt_off=over.opt_off)
    assert e.value.code == nsx.NSX_EINVAL


def test_tx_layout_host_matches_its_restatement():
    """nsx_tx_layout_host: out_off[i] = Σ_{j<i} round_up4(ip_hdr_len + wire_j), with and without options, option
    lengths that take the reference's padding (tcp.go:118-121) included; ip_hdr_len outside {20, 40} is NSX_EINVAL."""
    rng = np.random.default_rng(0x7A)
    n = 400
    lens = rng.integers(0, 3000, n)
    keys = sorted(_tx.OPT_SETS)
    ob = [_tx.opt_bytes(rng, keys[i % len(keys)]) if i % 3 else b"" for i in range(n)]
    for ipver in (4, 6):
        for opts in (None, ob):
            c = _tx.Case(rng, ipver, lens, opts=opts)
            got = nsx.tx_layout_host(c.data_off, c.opt_off, _tx.IPH[ipver])
            assert np.array_equal(got, c.packed())
            for i in range(0, n, 37):  # the frame lengths behind it: nsx_tcp_wire_len + the IP header
                assert int(c.flen[i]) == _tx.IPH[ipver] + nsx.tcp_wire_len(len(ob[i]) if opts else 0, int(lens[i]))
    c = _tx.Case(rng, 4, lens[:5])
    for bad in (0, 19, 21, 24, 60, 1 << 20):
        with pytest.raises(nsx.NsxError) as e:
            nsx.tx_layout_host(c.data_off, None, bad)
        assert e.value.code == nsx.NSX_EINVAL, bad
    L = nsx.lib()
    assert L.nsx_tx_layout_host(None, c.data_off.ctypes.data_as(ctypes.c_void_p), 5, 20, None) == nsx.NSX_EINVAL
    assert L.nsx_tx_layout_host(None, None, 5, 20, fake) == nsx.NSX_EINVAL
    one = np.full(1, 77, np.uint64)
    assert L.nsx_tx_layout_host(None, None, 0, 40, one.ctypes.data_as(ctypes.c_void_p)) == 0 and one[0] == 0


def test_tx_binding_checks_extents_before_the_c_call():
    """Every tensor's extent is checked before the C call (CPU tensors here: a well-formed one is then refused as
    not on a device): short src, dst, ident, ttl, tclass, flow, out or offsets raise ValueError."""
    import torch
    n = 3
    offs = torch.tensor([0, 10, 20, 30], dtype=torch.int64)
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8)  # noqa: E731
    fields = {k: torch.zeros(n, dtype={1: torch.uint8, 2: torch.int16, 4: torch.int32}[s]) for k, s in nsx.BUILD_FIELDS}
    for ipver, fn in ((4, nsx.tx_ipv4_tcp_build_dev), (6, nsx.tx_ipv6_tcp_build_dev)):
        alen = 4 if ipver == 4 else 16
        ip = {"src": u8(alen * n), "dst": u8(alen * n), "ident": torch.zeros(n, dtype=torch.int16), "ttl": u8(n),
              "tclass": u8(n), "flow": torch.zeros(n, dtype=torch.int32)}
        build = dict(data=u8(30), data_off=offs, out=u8(400), out_off=offs)
        cases = [
            (dict(ip, src=u8(alen * n - 1)), fields, build, " src"),
            (dict(ip, dst=u8(alen * n - 1)), fields, build, " dst"),
            (dict(ip, src=None), fields, build, "'src' missing"),
            (dict(ip, ident=torch.zeros(n - 1, dtype=torch.int16)), fields, build, " ident"),
            (dict(ip, ident=torch.zeros(n, dtype=torch.int32)), fields, build, "2-byte elements"),
            (dict(ip, ttl=u8(n - 1)), fields, build, " ttl"),
            (dict(ip, tclass=u8(n - 1)), fields, build, " tclass"),
            (dict(ip, flow=torch.zeros(n - 1, dtype=torch.int32)), fields, build, " flow"),
            (ip, dict(fields, window=torch.zeros(n - 1, dtype=torch.int16)), build, " window"),
            (ip, dict(fields, seq_num=None), build, "'seq_num' missing"),
            (ip, fields, dict(build, out_off=offs[:3]), " out_off"),
            (ip, fields, dict(build, out=u8(n * (40 if ipver == 4 else 60) - 1)), " out:"),
            (ip, fields, dict(build, raw=torch.zeros(n - 1, dtype=torch.int16)), " raw"),
            (ip, fields, dict(build, opt_off=offs), "opt_off given without opts"),
            (ip, fields, dict(build, opt_off=offs[:3], opts=u8(8)), " opt_off"),
            (ip, fields, build, "device"),
        ]
        for ipd, f, b, msg in cases:
            with pytest.raises(ValueError) as e:
                fn(ipd, f, **b)
            assert msg in str(e.value), (msg, str(e.value))
    # host wrappers: the arrays are host arrays, the same extents
    for ipver in (4, 6):
        fn = getattr(nsx, f"tx_ipv{ipver}_tcp_build_host")
        c = _host_case(ipver)
        total = int(c.packed()[-1])
        for kw, msg in ((dict(ip=dict(c.ip, src=c.ip["src"][:2])), " src"),
                        (dict(ip=dict(c.ip, dst=c.ip["dst"][:2])), " dst"),
                        (dict(ip=dict(c.ip, ident=c.ip["ident"][:2])), " ident"),
                        (dict(ip=dict(c.ip, ttl=c.ip["ttl"][:2])), " ttl"),
                        (dict(ip=dict(c.ip, tclass=c.ip["tclass"][:2])), " tclass"),
                        (dict(ip=dict(c.ip, flow=c.ip["flow"][:2])), " flow"),
                        (dict(ip=dict(c.ip, dst=None)), "'dst' missing"),
                        (dict(fields=dict(c.fields, ack_num=c.fields["ack_num"][:2])), " ack_num"),
                        (dict(data=c.data[:29]), "data_off ends at 30"),
                        (dict(out=np.zeros(total - 1, np.uint8)), f"out_off ends at {total}"),
                        (dict(out_off=c.packed()[:3]), " out_off"),
                        (dict(opt_off=np.zeros(4, np.uint64)), "opt_off given without opts"),
                        (dict(out=np.zeros(2 * total, np.uint8)[::2]), "C-contiguous uint8")):
            args = dict(ip=c.ip, fields=c.fields, data=c.data, data_off=c.data_off)
            args.update(kw)
            with pytest.raises(ValueError) as e:
                fn(**args)
            assert msg in str(e.value), (msg, str(e.value))


def _mixed_case(rng, ipver, n=96):
    keys = sorted(_tx.OPT_SETS)
    lens = rng.integers(0, 1700, n)
    lens[:6] = [0, 1, 2, 3, 4, 1480]
    ob = [_tx.opt_bytes(rng, keys[i % len(keys)]) if i % 2 else b"" for i in range(n)]
    return _tx.Case(rng, ipver, lens, opts=ob, lead=3)


@pytest.mark.parametrize("ipver", [4, 6])
def test_expected_frames_equal_the_oracle_frames(ipver):
    """tests/_tx.py agrees byte for byte with O.ipv4_tcp_frame / O.ipv6_tcp_frame (the frames the receive tests are
    built from) on 96 frames, half of them with options; its vectorised IPv4 header checksum equals O.go_checksum on
    every header of the batch; and the padding after each frame is zero over a sentinel buffer."""
    rng = np.random.default_rng(0x7B + ipver)
    c = _mixed_case(rng, ipver)
    off = c.packed()
    buf, raw = _tx.expected(c, off, fill=0xAB)
    iph = _tx.IPH[ipver]
    hdr = _tx.ip_headers(c)
    for i in range(c.n):
        o, L = int(off[i]), int(c.flen[i])
        seg = buf[o + iph:o + L].tobytes()
        src, dst = c.ip["src"][i].tobytes(), c.ip["dst"][i].tobytes()
        if ipver == 4:
            want = O.ipv4_tcp_frame(seg, src, dst, int(c.ip["ident"][i]), int(c.ip["ttl"][i]))
            z = bytearray(hdr[i].tobytes())
            z[10:12] = b"\0\0"
            assert int(_tx.hdr_checksum(np.frombuffer(bytes(z), np.uint8)[None, :])[0]) == O.go_checksum(b"", bytes(z))
        else:
            want = O.ipv6_tcp_frame(seg, src, dst, int(c.ip["ttl"][i]), int(c.ip["flow"][i]), int(c.ip["tclass"][i]))
        assert buf[o:o + L].tobytes() == want, i
        assert not buf[o + L:int(off[i + 1])].any()
        z = bytearray(seg)
        z[16:18] = b"\0\0"
        ph = (O.ipv4_pseudo_header if ipver == 4 else O.ipv6_pseudo_header)(src, dst, 6, len(seg))
        assert int(raw[i]) == O.go_checksum(ph, bytes(z)) != 0


@pytest.mark.parametrize("ipver", [4, 6])
def test_expected_frames_pass_the_receive_oracle(ipver):
    """Every expected frame is valid to the receive oracle (O.c_rx_ipv4_tcp / O.c_rx_ipv6_tcp), with frame lengths
    that are multiples of 4 so that the packed layout is the receive pass's offsets."""
    rng = np.random.default_rng(0x7D + ipver)
    n = 300
    lens = 4 * rng.integers(0, 500, n)
    keys = ["mss", "nop_nop_k2len10", "k2len40"]  # 4-aligned headers
    ob = [_tx.opt_bytes(rng, keys[i % 3]) if i % 3 == 0 else b"" for i in range(n)]
    c = _tx.Case(rng, ipver, lens, opts=ob)
    assert not (c.flen % 4).any()
    off = c.packed()
    buf, raw = _tx.expected(c, off)
    res = O.c_rx_ipv4_tcp(buf, off) if ipver == 4 else O.c_rx_ipv6_tcp(buf, off)
    want_mask = np.packbits(np.ones(n, np.uint8), bitorder="little")
    assert np.array_equal(res[0].view(np.uint8)[:want_mask.size], want_mask)
    assert (res[-1] == 0xFFFF).all()
    if ipver == 4:
        assert (res[1] == 0xFFFF).all()
