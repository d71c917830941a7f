"""Segmentation offload's boundary (nsx_tso_*), on any host: the symbols, the frame-map calls against their numpy
restatement, every NSX_EINVAL, validation before any device work, the binding's extent checks, and the self-checks of
the expected-frame helper tests/_tso.py that the GPU tests (tests/test_gpu_tso.py) compare against."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nsx
import _tso
import _tx
from oracle import csum_oracle as O

DEV_CALLS = ("nsx_tso_ipv4_tcp_build_dev", "nsx_tso_ipv6_tcp_build_dev")
HOST_CALLS = ("nsx_tso_ipv4_tcp_build_host", "nsx_tso_ipv6_tcp_build_host")
MAP_CALLS = ("nsx_tso_count_host", "nsx_tso_layout_host")
fake = ctypes.c_void_p(0x1000)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSS_SET = (1, 536, 1460, 1461, 65535)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _cut_lengths(mss):
    """0, 1, mss − 1, mss, mss + 1, 3·mss and 3·mss ± 1 (the cut points of one super-segment)."""
    return sorted({0, 1, max(mss - 1, 0), mss, mss + 1, 3 * mss - 1, 3 * mss, 3 * mss + 1})


def test_tso_symbols_are_declared_and_exported(tmp_path):
    """nsx_csum.h declares the two frame-map calls and the four build calls, nsx_tx_tune.h their four _tuned twins;
    the library exports all ten; NSX_ABI_VERSION stays 2; the header states the flag rule and that SYN is copied;
    and a plain C caller compiles against them and gets NSX_EINVAL / NSX_OK from the validation."""
    inc = os.path.join(ROOT, "include")
    text = open(os.path.join(inc, "nsx_csum.h")).read()
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)  # noqa: E731
    plain = set(re.findall(r"^int (nsx_tso_[a-z_0-9]+)\(", strip(text), flags=re.M))
    tuned = set(re.findall(r"^int (nsx_tso_[a-z_0-9]+)\(", strip(open(os.path.join(inc, "nsx_tx_tune.h")).read()),
                           flags=re.M))
    assert plain == set(DEV_CALLS) | set(HOST_CALLS) | set(MAP_CALLS)
    assert tuned == {f + "_tuned" for f in DEV_CALLS + HOST_CALLS}
    out = subprocess.run(["nm", "-D", "--defined-only", nsx.LIB_PATH], capture_output=True, text=True).stdout
    assert plain | tuned <= set(re.findall(r" T (nsx_\w+)", out))
    assert nsx.abi_version() == 2
    for word in ("tcp_gso_segment", "SYN is merely copied", "gso_size", "no segmenting form of the IP-less"):
        assert word in re.sub(r"\s*\n \*\s*", " ", text), word
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include "nsx_tune.h"
int main(void) {
    nsx_ip_hdr_soa ip = {0};
    nsx_tcp_hdr_soa tcp = {0};
    nsx_tune t = {0};
    uint64_t doff[2] = {0, 3000}, first[2] = {9, 9}, out[4];
    uint32_t mss[1] = {1460}, seg[3];
    if (nsx_tso_count_host(doff, mss, 1, first) != NSX_OK || first[0] != 0 || first[1] != 3) return 1;
    if (nsx_tso_layout_host(0, doff, mss, first, 1, 20, seg, out) != NSX_OK || out[3] != 2 * 1500 + 120) return 2;
    if (nsx_tso_ipv4_tcp_build_dev_tuned(&ip, &tcp, 0, 0, 0, doff, 0, mss, 1, first, seg, 3, 0, out, 0, 0, &t)
        != NSX_EINVAL) return 3;
    if (nsx_tso_ipv6_tcp_build_host_tuned(&ip, &tcp, 0, 0, 0, doff, mss, 1, first, seg, 3, 0, out, 0, 0, &t)
        != NSX_EINVAL) return 4;
    if (nsx_tso_ipv6_tcp_build_dev(&ip, &tcp, 0, 0, 0, doff, 0, mss, 1, first, seg, 0, 0, out, 0, 0) != NSX_OK) return 5;
    return nsx_tso_ipv4_tcp_build_host(&ip, &tcp, 0, 0, 0, doff, mss, 1, first, seg, 0, 0, out, 0, 0) == NSX_OK ? 0 : 6;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(nsx.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I", inc, "-L", libdir, "-lnsx_csum",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- the frame map
@pytest.mark.parametrize("mss", MSS_SET)
def test_tso_count_and_layout_match_their_restatement(mss):
    """Frame counts max(1, ceil(len / mss)) as a prefix sum, each frame's super-segment, and the packed slots of the
    expanded batch (= nsx_tx_layout_host over the expansion), at every cut point of every mss, with and without
    options, for both IP header lengths."""
    rng = np.random.default_rng(0x150 + mss)
    lens = _cut_lengths(mss) + [int(x) for x in rng.integers(0, 4 * mss + 2, 8)]
    keys = sorted(_tx.OPT_SETS)
    ob = [_tx.opt_bytes(rng, keys[i % len(keys)]) if i % 3 else b"" for i in range(len(lens))]
    for ipver in (4, 6):
        for opts in (None, ob):
            b = _tso.Batch(rng, ipver, lens, mss, opts=opts, lead=1)
            first = nsx.tso_count_host(b.sup.data_off, b.mss)
            want_cnt = [max(1, -(-L // mss)) for L in lens]
            assert np.array_equal(np.diff(first), want_cnt) and first[0] == 0
            assert np.array_equal(first, b.first)
            seg, off = nsx.tso_layout_host(b.sup.data_off, b.mss, first, b.sup.opt_off, _tx.IPH[ipver])
            assert np.array_equal(seg, b.seg) and np.array_equal(off, b.off)
            assert np.array_equal(seg, np.repeat(np.arange(len(lens)), want_cnt))
            c = _tso.expand(b)
            assert np.array_equal(off, nsx.tx_layout_host(c.data_off, c.opt_off, _tx.IPH[ipver]))
            assert np.array_equal(off, c.packed())
            assert int(np.diff(c.data_off).sum()) == sum(lens) and int(np.diff(c.data_off).max()) <= mss


def test_tso_count_and_layout_mixed_mss():
    rng = np.random.default_rng(0x15F)
    mss = np.array(MSS_SET * 4, np.uint32)
    lens = rng.integers(0, 70000, mss.size)
    b = _tso.Batch(rng, 4, lens, mss)
    first = nsx.tso_count_host(b.sup.data_off, mss)
    assert np.array_equal(first, b.first)
    seg, off = nsx.tso_layout_host(b.sup.data_off, mss, first, None, 20)
    assert np.array_equal(seg, b.seg) and np.array_equal(off, b.off)


def test_tso_count_and_layout_refuse_bad_arguments():
    """nsx_tso_count_host: an mss of 0, decreasing offsets, n >= 2^32, NULL arrays. nsx_tso_layout_host: the same,
    decreasing option offsets, ip_hdr_len other than 20 or 40, and a frame_first that is not nsx_tso_count_host's;
    a refused layout call writes nothing."""
    L = nsx.lib()
    doff = np.array([0, 3000, 3000, 9000], np.uint64)
    mss = np.array([1460, 1460, 1000], np.uint32)
    first = np.zeros(4, np.uint64)
    assert L.nsx_tso_count_host(_p(doff), _p(mss), 3, _p(first)) == 0
    assert first.tolist() == [0, 3, 4, 10]
    E = nsx.NSX_EINVAL
    assert L.nsx_tso_count_host(_p(doff), _p(np.array([1460, 0, 1000], np.uint32)), 3, _p(first)) == E
    assert L.nsx_tso_count_host(_p(np.array([0, 3000, 2999, 9000], np.uint64)), _p(mss), 3, _p(first)) == E
    assert L.nsx_tso_count_host(_p(doff), _p(mss), 1 << 32, _p(first)) == E
    assert L.nsx_tso_count_host(None, _p(mss), 3, _p(first)) == E
    assert L.nsx_tso_count_host(_p(doff), None, 3, _p(first)) == E
    assert L.nsx_tso_count_host(_p(doff), _p(mss), 3, None) == E
    one = np.full(1, 77, np.uint64)
    assert L.nsx_tso_count_host(None, None, 0, _p(one)) == 0 and one[0] == 0

    seg = np.full(10, 0xEEEE, np.uint32)
    off = np.full(11, 0xEEEE, np.uint64)
    ooff = np.array([0, 4, 4, 12], np.uint64)

    def lay(opt_off=ooff, data_off=doff, m=mss, f=first, n=3, iph=20, s=seg, o=off):
        return L.nsx_tso_layout_host(_p(opt_off), _p(data_off), _p(m), _p(f), n, iph, _p(s), _p(o))

    bad = [dict(m=np.array([1460, 0, 1000], np.uint32)), dict(data_off=np.array([0, 3000, 2999, 9000], np.uint64)),
           dict(opt_off=np.array([0, 4, 3, 12], np.uint64)), dict(n=1 << 32), dict(data_off=None), dict(m=None),
           dict(f=None), dict(o=None), dict(s=None), dict(iph=0), dict(iph=24), dict(iph=60),
           dict(f=np.array([0, 3, 4, 11], np.uint64)), dict(f=np.array([0, 2, 4, 10], np.uint64)),
           dict(f=np.array([1, 3, 4, 10], np.uint64)), dict(f=np.array([0, 3, 5, 10], np.uint64))]
    for kw in bad:
        assert lay(**kw) == E, kw
        assert (seg == 0xEEEE).all() and (off == 0xEEEE).all(), kw
    assert lay() == 0 and seg.tolist() == [0, 0, 0, 1, 2, 2, 2, 2, 2, 2]
    assert lay(opt_off=None) == 0 and off[1] == 1500 and off[4] - off[3] == 40
    # the binding reports them as NsxError
    for fn, args in ((nsx.tso_count_host, (doff, [1460, 0, 1000])),
                     (nsx.tso_layout_host, (doff, mss, [0, 3, 4, 11])),
                     (nsx.tso_layout_host, (doff, mss, first, None, 24))):
        with pytest.raises(nsx.NsxError) as e:
            fn(*args)
        assert e.value.code == E


# ---------------------------------------------------------------- device calls: validation
def _soas(ip_null=(), tcp_null=()):
    ip = nsx.IpHdrSoA(*[None if k in ip_null else 0x1000 for k in nsx.IP_FIELDS])
    tcp = nsx.TcpHdrSoA(*[None if k in tcp_null else 0x1000 for k, _ in nsx.BUILD_FIELDS])
    return ip, tcp


def _dev_call(name, ip, tcp, n=4, nf=9, tuned=False, **kw):
    """One raw device call with fake pointers (validation must refuse or pass it before any device work)."""
    a = dict(opts=None, opt_off=None, data=fake, data_off=fake, data_bytes=64, mss=fake, first=fake, seg=fake,
             out=fake, out_off=fake, raw=None)
    a.update(kw)
    args = [None if ip is None else ctypes.byref(ip), None if tcp is None else ctypes.byref(tcp), a["opts"],
            a["opt_off"], a["data"], a["data_off"], a["data_bytes"], a["mss"], n, a["first"], a["seg"], nf, a["out"],
            a["out_off"], a["raw"], None]
    if tuned:
        return getattr(nsx.lib(), name + "_tuned")(*args, ctypes.byref(nsx.Tune(run_segs=16)))
    return getattr(nsx.lib(), name)(*args)


def test_tso_device_calls_validate_before_any_device_work():
    """n_frames == 0 is a no-op; the transmit pass's NULL checks plus the frame map's (mss, frame_first, frame_seg),
    fewer frames than super-segments, no super-segments, n >= 2^32: NSX_EINVAL; the optional ident / ttl / tclass /
    flow / offset may be NULL; and with no GPU every entry point and _tuned twin then answers NSX_ENODEV."""
    ip, tcp = _soas()
    for name in DEV_CALLS:
        for tuned in (False, True):
            assert _dev_call(name, None, None, nf=0, tuned=tuned) == 0
            assert _dev_call(name, None, tcp, tuned=tuned) == nsx.NSX_EINVAL
            assert _dev_call(name, ip, None, tuned=tuned) == nsx.NSX_EINVAL
            for k in ("src", "dst"):
                assert _dev_call(name, _soas(ip_null=(k,))[0], tcp, tuned=tuned) == nsx.NSX_EINVAL, k
            for k, _ in nsx.BUILD_FIELDS:
                if k != "offset":
                    assert _dev_call(name, ip, _soas(tcp_null=(k,))[1], tuned=tuned) == nsx.NSX_EINVAL, k
            for kw in (dict(out=None), dict(out_off=None), dict(data_off=None), dict(data=None), dict(mss=None),
                       dict(first=None), dict(seg=None), dict(opt_off=fake, opts=None), dict(n=4, nf=3), dict(n=0),
                       dict(n=1 << 32, nf=1 << 33)):
                assert _dev_call(name, ip, tcp, tuned=tuned, **kw) == nsx.NSX_EINVAL, kw
            if nsx.device_count() == 0:
                assert _dev_call(name, ip, tcp, tuned=tuned) == nsx.NSX_ENODEV
                opt = _soas(ip_null=("ident", "ttl", "tclass", "flow"), tcp_null=("offset",))
                assert _dev_call(name, *opt, tuned=tuned) == nsx.NSX_ENODEV


# ---------------------------------------------------------------- host calls: validation
def _host_batch(ipver, lens=(10, 3000, 0), mss=1460, opts=None):
    return _tso.Batch(np.random.default_rng(0x160 + ipver), ipver, list(lens), mss, opts=opts)


def test_tso_host_calls_validate_before_any_device():
    """A well-formed batch is NSX_ENODEV on a GPU-less host; a malformed one NSX_EINVAL everywhere: an mss of 0,
    decreasing offsets, a frame_first or frame_seg that is not the frame map's, slots that are misaligned, too
    short or decreasing, NULL structs and members; n_frames == 0 returns 0."""
    for ipver, name in zip((4, 6), HOST_CALLS):
        fn = getattr(nsx, f"tso_ipv{ipver}_tcp_build_host")
        b = _host_batch(ipver)
        s = b.sup
        assert b.nf == 5
        if nsx.device_count() == 0:
            for tune in (None, dict(shards_per_device=3), dict(chunk_bytes=2048)):
                with pytest.raises(nsx.NsxError) as e:
                    fn(s.ip, s.fields, s.data, s.data_off, b.mss, tune=tune)
                assert e.value.code == nsx.NSX_ENODEV
        total = int(b.off[-1])
        out = np.zeros(total + 16, np.uint8)
        shifted, short, back = b.off + np.uint64(2), b.off.copy(), b.off.copy()
        short[2] -= np.uint64(4)
        back[3] = back[1]
        wrong_seg = b.seg.copy()
        wrong_seg[2] = 2
        for kw in (dict(mss=np.array([1460, 0, 1460], np.uint32)),
                   dict(data_off=np.array([0, 10, 5, 3010], np.uint64)),
                   dict(frame_first=np.array([0, 1, 3, 5], np.uint64)),
                   dict(frame_first=np.array([0, 2, 4, 5], np.uint64)),
                   dict(frame_seg=wrong_seg), dict(out_off=shifted), dict(out_off=short), dict(out_off=back)):
            args = dict(ip=s.ip, fields=s.fields, data=s.data, data_off=s.data_off, mss=b.mss, frame_first=b.first,
                        frame_seg=b.seg, out_off=b.off, out=out)
            args.update(kw)
            with pytest.raises(nsx.NsxError) as e:
                fn(**args)
            assert e.value.code == nsx.NSX_EINVAL, kw
        L = nsx.lib()

        def call(ip, tcp, nf=5, n=3, tuned=False, mss=b.mss, first=b.first, seg=b.seg):
            args = [None if ip is None else ctypes.byref(ip), None if tcp is None else ctypes.byref(tcp), None, None,
                    _p(s.data), _p(s.data_off), _p(mss), n, _p(first), _p(seg), nf, _p(out), _p(b.off), None, 0]
            return getattr(L, name + "_tuned")(*args, None) if tuned else getattr(L, name)(*args)

        def soas(ip_null=(), tcp_null=()):
            return (nsx.IpHdrSoA(*[None if k in ip_null else s.ip[k].ctypes.data for k in nsx.IP_FIELDS]),
                    nsx.TcpHdrSoA(*[None if k in tcp_null else s.fields[k].ctypes.data for k, _ in nsx.BUILD_FIELDS]))

        ip, tcp = soas()
        for tuned in (False, True):
            assert call(None, None, nf=0, tuned=tuned) == 0
            assert call(None, tcp, tuned=tuned) == nsx.NSX_EINVAL
            assert call(ip, None, tuned=tuned) == nsx.NSX_EINVAL
            assert call(soas(ip_null=("src",))[0], tcp, tuned=tuned) == nsx.NSX_EINVAL
            assert call(soas(ip_null=("dst",))[0], tcp, tuned=tuned) == nsx.NSX_EINVAL
            assert call(ip, soas(tcp_null=("window",))[1], tuned=tuned) == nsx.NSX_EINVAL
            for kw in (dict(mss=None), dict(first=None), dict(seg=None), dict(nf=4), dict(nf=6), dict(n=0),
                       dict(n=1 << 32)):
                assert call(ip, tcp, tuned=tuned, **kw) == nsx.NSX_EINVAL, kw


@pytest.mark.parametrize("ipver", [4, 6])
def test_tso_host_calls_refuse_a_frame_that_does_not_fit_its_length_field(ipver):
    """A frame whose TCP part exceeds the IP length field — an mss one byte too large for it (IPv4 65496, IPv6
    65516, no options) under a super-segment that fills a frame — is NSX_EINVAL before any device is touched; the
    same super-segment at one byte less per frame passes validation."""
    fn = getattr(nsx, f"tso_ipv{ipver}_tcp_build_host")
    top = _tx.WIRE_MAX[ipver] - 20
    over = _host_batch(ipver, lens=(10, 2 * (top + 1), 10), mss=top + 1)
    s = over.sup
    with pytest.raises(nsx.NsxError) as e:
        fn(s.ip, s.fields, s.data, s.data_off, over.mss)
    assert e.value.code == nsx.NSX_EINVAL
    # the same mss is fine while no frame is that long
    ok = [_host_batch(ipver, lens=(10, 2 * (top + 1), 10), mss=top), _host_batch(ipver, lens=(10, top, 10), mss=top + 1)]
    for b in ok:
        s = b.sup
        if nsx.device_count() == 0:
            with pytest.raises(nsx.NsxError) as e:
                fn(s.ip, s.fields, s.data, s.data_off, b.mss)
            assert e.value.code == nsx.NSX_ENODEV
        else:
            got, raw = fn(s.ip, s.fields, s.data, s.data_off, b.mss)
            want, wraw, _ = _tso.expected(b)
            assert np.array_equal(got, want) and np.array_equal(raw, wraw)
    # with options: the option bytes and their padding count (1 option byte + 1 pad: a 22-byte header)
    rng = np.random.default_rng(0x16A)
    ob = [b"", _tx.opt_bytes(rng, "nop"), b""]
    over = _host_batch(ipver, lens=(10, 3 * (top - 1), 10), mss=top - 1, opts=ob)
    s = over.sup
    with pytest.raises(nsx.NsxError) as e:
        fn(s.ip, s.fields, s.data, s.data_off, over.mss, opts=s.opts, opt_off=s.opt_off)
    assert e.value.code == nsx.NSX_EINVAL


# ---------------------------------------------------------------- the binding's extent checks
def test_tso_binding_checks_extents_before_the_c_call():
    """Every tensor's extent is checked before the C call (CPU tensors here: a well-formed call is then refused as
    not on a device): short per-super-segment arrays, a frame_seg shorter than n_frames, an out_off shorter than
    n_frames + 1, a raw shorter than n_frames raise ValueError; the host wrappers check the same on host arrays."""
    import torch
    n, nf = 3, 5
    doff = torch.tensor([0, 10, 3010, 3010], dtype=torch.int64)
    first = torch.tensor([0, 1, 4, 5], dtype=torch.int64)
    seg = torch.tensor([0, 1, 1, 1, 2], dtype=torch.int32)
    ooff = torch.tensor([0, 52, 1552, 3052, 3172, 3212], dtype=torch.int64)
    mss = torch.full((n,), 1460, dtype=torch.int32)
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8)  # noqa: E731
    fields = {k: torch.zeros(n, dtype={1: torch.uint8, 2: torch.int16, 4: torch.int32}[s]) for k, s in nsx.BUILD_FIELDS}
    for ipver, fn in ((4, nsx.tso_ipv4_tcp_build_dev), (6, nsx.tso_ipv6_tcp_build_dev)):
        alen = 4 if ipver == 4 else 16
        ip = {"src": u8(alen * n), "dst": u8(alen * n), "ident": torch.zeros(n, dtype=torch.int16), "ttl": u8(n),
              "tclass": u8(n), "flow": torch.zeros(n, dtype=torch.int32)}
        build = dict(data=u8(3010), data_off=doff, mss=mss, frame_first=first, frame_seg=seg, out=u8(4000),
                     out_off=ooff)
        cases = [
            (dict(ip, src=u8(alen * n - 1)), fields, build, " src"),
            (dict(ip, dst=None), fields, build, "'dst' missing"),
            (dict(ip, ident=torch.zeros(n - 1, dtype=torch.int16)), fields, build, " ident"),
            (dict(ip, flow=torch.zeros(n - 1, dtype=torch.int32)), fields, build, " flow"),
            (ip, dict(fields, window=torch.zeros(n - 1, dtype=torch.int16)), build, " window"),
            (ip, dict(fields, control=None), build, "'control' missing"),
            (ip, fields, dict(build, mss=mss[:2]), " mss"),
            (ip, fields, dict(build, mss=torch.zeros(n, dtype=torch.int64)), "4-byte elements"),
            (ip, fields, dict(build, frame_first=first[:3]), " frame_first"),
            (ip, fields, dict(build, frame_seg=seg[:4]), " frame_seg"),
            (ip, fields, dict(build, frame_seg=torch.zeros(nf, dtype=torch.int64)), "4-byte elements"),
            (ip, fields, dict(build, out_off=ooff[:5], n_frames=nf), " out_off"),
            (ip, fields, dict(build, n_frames=2), "2 frames for 3 super-segments"),
            (ip, fields, dict(build, out=u8(nf * (40 if ipver == 4 else 60) - 1)), " out:"),
            (ip, fields, dict(build, raw=torch.zeros(nf - 1, dtype=torch.int16)), " raw"),
            (ip, fields, dict(build, opt_off=doff), "opt_off given without opts"),
            (ip, fields, dict(build, opt_off=doff[:3], opts=u8(8)), " opt_off"),
            (ip, fields, dict(build, raw=torch.zeros(nf, dtype=torch.int16)), "device"),
        ]
        for ipd, f, b, msg in cases:
            with pytest.raises(ValueError) as e:
                fn(ipd, f, **b)
            assert msg in str(e.value), (msg, str(e.value))
    for ipver in (4, 6):
        fn = getattr(nsx, f"tso_ipv{ipver}_tcp_build_host")
        b = _host_batch(ipver)
        s = b.sup
        total = int(b.off[-1])
        for kw, msg in ((dict(ip=dict(s.ip, src=s.ip["src"][:2])), " src"),
                        (dict(ip=dict(s.ip, ident=s.ip["ident"][:2])), " ident"),
                        (dict(ip=dict(s.ip, dst=None)), "'dst' missing"),
                        (dict(fields=dict(s.fields, ack_num=s.fields["ack_num"][:2])), " ack_num"),
                        (dict(mss=b.mss[:2]), " mss"),
                        (dict(frame_first=b.first[:3]), " frame_first"),
                        (dict(frame_seg=b.seg[:4]), " frame_seg"),
                        (dict(out_off=b.off[:5]), " out_off"),
                        (dict(data=s.data[:3009]), "data_off ends at 3010"),
                        (dict(out=np.zeros(total - 1, np.uint8)), f"out_off ends at {total}"),
                        (dict(opt_off=np.zeros(4, np.uint64)), "opt_off given without opts"),
                        (dict(out=np.zeros(2 * total, np.uint8)[::2]), "C-contiguous uint8")):
            args = dict(ip=s.ip, fields=s.fields, data=s.data, data_off=s.data_off, mss=b.mss)
            args.update(kw)
            with pytest.raises(ValueError) as e:
                fn(**args)
            assert msg in str(e.value), (msg, str(e.value))


# ---------------------------------------------------------------- tests/_tso.py held to the oracle
def _mixed_batch(rng, ipver, n=40, four=False):
    """About 40 super-segments: every cut point of several mss values, flags that exercise the FIN / PSH / CWR rule,
    sequence numbers and idents about to wrap, half with options."""
    mss = np.array([(1460, 536, 3, 1461, 8960)[i % 5] for i in range(n)], np.uint32)
    if four:
        mss = np.array([(1460, 536, 8, 1448, 8960)[i % 5] for i in range(n)], np.uint32)
    lens = np.array([int(rng.integers(0, 5 * m + 2)) for m in mss])
    for i, m in enumerate(mss[:16]):
        lens[i] = _cut_lengths(int(m))[i % 8]
    if four:
        lens = 4 * (lens // 4)
    keys = ["mss", "nop_nop_k2len10", "k2len40"] if four else sorted(_tx.OPT_SETS)
    ob = [_tx.opt_bytes(rng, keys[i % len(keys)]) if i % 2 else b"" for i in range(n)]
    b = _tso.Batch(rng, ipver, lens, mss, opts=ob, lead=0 if four else 3)
    b.sup.fields["control"][:] = np.resize(np.array([0xFF, 0x19, 0x89, 0x18, 0x11, 0x90, 0x80, 0x02], np.uint8), n)
    b.sup.fields["seq_num"][-4:] = [0xFFFFFFFF, 0xFFFFFFFF - 1460, 0xFFFFF000, 0]
    b.sup.ip["ident"][-4:] = [0xFFFF, 0xFFFE, 0xFFF0, 0]
    return b


@pytest.mark.parametrize("ipver", [4, 6])
def test_expansion_equals_the_oracle_frames(ipver):
    """Frame by frame, from the super-segment's own arrays and the rules stated in plain Python — slice, seq + j·mss
    mod 2^32, FIN / PSH on the last frame only, CWR on the first only, ident + j mod 2^16, everything else copied —
    serialised by O.Segment and O.ipv4_tcp_frame / O.ipv6_tcp_frame: the expected buffer of tests/_tso.py holds
    exactly those frames, zero padding after each, and its raw sums are the pseudo-header sums."""
    rng = np.random.default_rng(0x170 + ipver)
    b = _mixed_batch(rng, ipver)
    s = b.sup
    buf, raw, c = _tso.expected(b, fill=0xAB)
    assert c.n == b.nf and b.nf > 2 * b.n
    iph = _tx.IPH[ipver]
    f = 0
    for i in range(b.n):
        db, de, m = int(s.data_off[i]), int(s.data_off[i + 1]), int(b.mss[i])
        cnt = max(1, -(-(de - db) // m))
        ob = s.opts[int(s.opt_off[i]):int(s.opt_off[i + 1])].tobytes()
        src, dst = s.ip["src"][i].tobytes(), s.ip["dst"][i].tobytes()
        for j in range(cnt):
            ctl = int(s.fields["control"][i])
            if j != cnt - 1:
                ctl &= ~0x09
            if j != 0:
                ctl &= ~0x80
            pay = s.data[min(db + j * m, de):min(db + (j + 1) * m, de)].tobytes()
            hdr_len = 20 + len(ob) + ((20 + len(ob)) % 4 if ob else 0)
            z = bytearray(hdr_len + len(pay))  # tcp.go:98-128 laid out by hand: fields, options, padding, payload
            z[0:2] = int(s.fields["src_port"][i]).to_bytes(2, "big")
            z[2:4] = int(s.fields["dst_port"][i]).to_bytes(2, "big")
            z[4:8] = ((int(s.fields["seq_num"][i]) + j * m) % (1 << 32)).to_bytes(4, "big")
            z[8:12] = int(s.fields["ack_num"][i]).to_bytes(4, "big")
            z[12] = int(s.fields["offset"][i])
            z[13] = ctl
            z[14:16] = int(s.fields["window"][i]).to_bytes(2, "big")
            z[18:20] = int(s.fields["urgent_ptr"][i]).to_bytes(2, "big")
            z[20:20 + len(ob)] = ob
            z[hdr_len:] = pay
            if ipver == 4:
                want = O.ipv4_tcp_frame(bytes(z), src, dst, (int(s.ip["ident"][i]) + j) % 65536, int(s.ip["ttl"][i]))
            else:
                want = O.ipv6_tcp_frame(bytes(z), src, dst, int(s.ip["ttl"][i]), int(s.ip["flow"][i]),
                                        int(s.ip["tclass"][i]))
            o, L = int(b.off[f]), len(want)
            assert L == int(c.flen[f]) and int(b.seg[f]) == i
            assert buf[o:o + L].tobytes() == want, (i, j)
            assert not buf[o + L:int(b.off[f + 1])].any()
            ph = (O.ipv4_pseudo_header if ipver == 4 else O.ipv6_pseudo_header)(src, dst, 6, len(z))
            assert int(raw[f]) == O.go_checksum(ph, bytes(z)) != 0
            f += 1
    assert f == b.nf
    # the flag, sequence and ident rules bite in this batch
    assert (c.fields["control"] != s.fields["control"][b.seg]).sum() > b.n
    assert (c.fields["seq_num"] < s.fields["seq_num"][b.seg]).any() and (c.ip["ident"] < s.ip["ident"][b.seg]).any()


@pytest.mark.parametrize("ipver", [4, 6])
def test_expansion_passes_the_receive_oracle(ipver):
    """Every expected frame is valid to the receive oracle (O.c_rx_ipv4_tcp / O.c_rx_ipv6_tcp): 4-multiple frame
    lengths, so that the packed layout is the receive pass's offsets."""
    rng = np.random.default_rng(0x178 + ipver)
    b = _mixed_batch(rng, ipver, four=True)
    buf, raw, c = _tso.expected(b)
    assert not (c.flen % 4).any()
    res = O.c_rx_ipv4_tcp(buf, b.off) if ipver == 4 else O.c_rx_ipv6_tcp(buf, b.off)
    want_mask = np.packbits(np.ones(b.nf, np.uint8), bitorder="little")
    assert np.array_equal(res[0].view(np.uint8)[:want_mask.size], want_mask)
    assert (res[-1] == 0xFFFF).all()
    if ipver == 4:
        assert (res[1] == 0xFFFF).all()


# ---------------------------------------------------------------- the cgo wrapper
def test_tso_cgo_wrapper_matches_the_header(tmp_path):
    """go/transport/tcp/tso_nsx.go under the type check of tests/test_cgo_shim.py: every C.nsx_* call names a
    declared, exported function with the header's argument count and exactly the header's argument types; every
    struct member it sets exists with that type; it calls both host entry points with pinned regions only; and the
    calls compile and link as C."""
    import test_cgo_shim as S
    gf = S.GoFile(os.path.join(S.GO_DIR, "tso_nsx.go"))
    protos = S.header_prototypes()
    exported = set(re.findall(r" T (nsx_\w+)", subprocess.run(
        ["nm", "-D", "--defined-only", nsx.LIB_PATH], capture_output=True, text=True).stdout))
    calls = gf.c_calls()
    assert {fn for fn, _ in calls} == set(HOST_CALLS) | {"nsx_tcp_wire_len", "nsx_strerror"}
    body = []
    for fn, args in calls:
        assert fn in protos and fn in exported, fn
        params = protos[fn][1]
        assert len(args) == len(params), (fn, len(args), len(params))
        for k, (a, want) in enumerate(zip(args, params)):
            assert S.go_to_c(gf.expr_type(a)) == want, (fn, k, a, want)
        if fn in HOST_CALLS:
            for a in args:
                assert a.startswith(("&ip", "&h", "(*C.uint8_t)(region(", "(*C.uint64_t)(region(",
                                     "(*C.uint32_t)(region(", "(*C.uint16_t)(region(", "optOffs", "C.uint64_t(n",
                                     "C.int(")), a
        decls = "".join(f"{S.go_to_c(gf.expr_type(a))} a{k} = 0; " for k, a in enumerate(args))
        body.append(f"    {{ {decls}(void){fn}({', '.join(f'a{k}' for k in range(len(args)))}); }}")
    src = re.sub(r"/\*.*?\*/", "", open(S.HEADER).read(), flags=re.S)
    members = {}
    for sbody, name in re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*(\w+)\s*;", src):
        for t, m in re.findall(r"((?:const\s+)?\w+\s*\*?)\s*(\w+)\s*;", sbody):
            members[(name, m)] = S._norm(t)
    checked = 0
    for var, typ in (("h", "nsx_tcp_hdr_soa"), ("ip", "nsx_ip_hdr_soa")):
        assert gf.vars[var] == "C." + typ
        for fld, rhs in re.findall(rf"\b{var}\.(\w+)\s*=\s*([^\n]+)", gf.src):
            assert S.go_to_c(gf.expr_type(rhs)) == members[(typ, fld)], (var, fld, rhs)
            checked += 1
    assert checked == 8 + 6
    text = open(gf.path).read()
    assert text.startswith("//go:build nsx") and '#include "nsx_csum.h"' in text
    csrc = tmp_path / "tso_calls.c"
    csrc.write_text("#include \"nsx_csum.h\"\nint main(int argc, char** argv) {\n    (void)argv;\n"
                    "    if (argc < 1000) return 0;\n" + "\n".join(body) + "\n    return 1;\n}\n")
    libdir = os.path.dirname(nsx.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-unused-variable", str(csrc), "-I",
                        os.path.join(ROOT, "include"), "-L", libdir, "-lnsx_csum", f"-Wl,-rpath,{libdir}",
                        "-o", str(tmp_path / "tso_calls")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
