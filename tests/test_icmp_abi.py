"""The ICMP family's boundary (nsx_icmp_*), on any host: the symbols, every NSX_EINVAL before NSX_ENODEV, the workspace
size, the binding's extent checks, and the numpy restatement tests/_icmp.py held to known answers worked out by hand,
to itself (every generated message verifies and quotes its frame; echo reply then verify passes and equals a rebuild
from scratch) and to the models that exist already (tests/_frag.py's statuses, tests/_nat.py's fold). The GPU tests
(tests/test_gpu_icmp_err.py, test_gpu_icmp_rx.py, test_gpu_icmp_echo.py, test_gpu_icmp_fuzz.py) compare the kernels
against tests/_icmp.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nsx
import _frag
import _icmp as M
import _nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ("nsx_icmp_err_work_bytes", "nsx_icmp_err_ipv4_dev", "nsx_icmp_err_ipv6_dev", "nsx_icmp_req_frag_dev",
         "nsx_icmp_req_ttl_ipv4_dev", "nsx_icmp_req_ttl_ipv6_dev", "nsx_icmp_rx_ipv4_verify_dev",
         "nsx_icmp_rx_ipv6_verify_dev", "nsx_icmp_echo_reply_ipv4_dev", "nsx_icmp_echo_reply_ipv6_dev")
TWINS = ("nsx_icmp_err_ipv4_dev_tuned", "nsx_icmp_err_ipv6_dev_tuned", "nsx_icmp_rx_ipv4_verify_dev_tuned",
         "nsx_icmp_rx_ipv6_verify_dev_tuned")
fake = ctypes.c_void_p(0x1000)
E, D, OK = nsx.NSX_EINVAL, nsx.NSX_ENODEV, nsx.NSX_OK
A4, B4 = bytes([10, 0, 0, 1]), bytes([192, 0, 2, 7])
A6, B6 = bytes([0x20, 1, 0xd, 0xb8] + [0] * 11 + [1]), bytes([0xfe, 0x80] + [0] * 13 + [9])


# ---------------------------------------------------------------- symbols
def test_icmp_symbols_are_declared_and_exported(tmp_path):
    """nsx_csum.h declares exactly the ten nsx_icmp_* calls and nsx_icmp_tune.h exactly the four _tuned twins; that
    header brings nsx_tune.h in, which keeps its 16 declarations, and no other tune header names the family; the
    library exports exactly the fourteen; the ABI version stays 2; the header states the contract; a plain C caller
    compiles with -Wall -Werror and gets the documented codes."""
    inc = os.path.join(ROOT, "include")
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)  # noqa: E731
    decl = r"^int\s+(nsx_icmp_[a-z_0-9]+)\("
    text = open(os.path.join(inc, "nsx_csum.h")).read()
    assert set(re.findall(decl, strip(text), flags=re.M)) == set(PLAIN)
    tune = open(os.path.join(inc, "nsx_icmp_tune.h")).read()
    assert set(re.findall(decl, strip(tune), flags=re.M)) == set(TWINS)
    assert '#include "nsx_tune.h"' in tune
    for h in ("nsx_tune.h", "nsx_tx_tune.h", "nsx_gro_tune.h", "nsx_udp_tune.h", "nsx_ugro_tune.h", "nsx_frag_tune.h"):
        assert "nsx_icmp_" not in open(os.path.join(inc, h)).read(), h
    assert len(re.findall(r"^int\s+nsx_\w+\(", strip(open(os.path.join(inc, "nsx_tune.h")).read()), flags=re.M)) == 16
    out = subprocess.run(["nm", "-D", "--defined-only", nsx.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (nsx_\w+)", out))
    assert {s for s in exported if s.startswith("nsx_icmp_")} == set(PLAIN) | set(TWINS)
    assert nsx.abi_version() == 2 and "NSX_ABI_VERSION 2 " in text
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for word in ("RFC 792, RFC 4443", "bits 16-31 must be 0", "RFC 1122 §3.2.2, RFC 1812 §4.3.2.7",
                 "MF alone does not count", "0, 8, 9, 10, 13, 14, 15, 16, 17, 18", "RFC 4443 §2.4(e)",
                 "Extension headers are not walked", "RFC 1812 §4.3.2.8 and RFC 4443 §2.4(f)", "q = min(len, Q)",
                 "ident = (ident0 + s) mod 2^16", "ICMP has no 0 -> 0xFFFF rule", "RFC 8200 §8.1 pseudo-header",
                 "Entries, offsets and bytes past the last one written stay as they were",
                 "min(n, max_out) entries of src_frame", "req = 3 | 4<<8, arg = d_mtu[i] & 0xFFFF",
                 "exactly the set the NAT rewrite refuses on TTL", "IHL*4 + 8 <= len",
                 "0xFFFF unless the bit is set", "the old dst becomes the new src",
                 "RFC 1624 eqn. 3 with the fold defined for nsx_nat_* above over the word at bytes 8-9",
                 "The address swap leaves both the header sum and the IPv6 pseudo-header sum unchanged",
                 "IP options and the payload are neither read nor written",
                 "stays wrong by the same one's-complement difference", "can be captured into a graph",
                 "frames may lie past 2^32 in d_base"):
        assert word in flat, word
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include "nsx_csum.h"
#include "nsx_icmp_tune.h"
int main(void) {
    nsx_icmp_err_cfg cfg = {{10, 0, 0, 1}, 64, 0, 100};
    nsx_icmp_err_out o = {0};
    nsx_tune t = {0};
    uint64_t need = 0, offs[2] = {0, 40}, mask[1] = {0};
    uint32_t req[1] = {11}, arg[1] = {0};
    uint8_t st[1] = {0};
    if (nsx_icmp_err_work_bytes(1000, &need) != NSX_OK || need < 4000) return 1;
    if (nsx_icmp_err_work_bytes(0xFFFFFFFFull, &need) != NSX_EINVAL || nsx_icmp_err_work_bytes(1, 0) != NSX_EINVAL) return 2;
    if (nsx_icmp_err_ipv4_dev(offs, offs, 1, req, arg, &cfg, &o, offs, 1 << 20, 0) != NSX_EINVAL) return 3;
    if (nsx_icmp_err_ipv6_dev_tuned(offs, offs, 1, req, arg, 0, &o, offs, 1 << 20, 0, &t) != NSX_EINVAL) return 4;
    cfg.ttl = 256;
    o.n_out = o.out_off = offs; o.out = st; o.src_frame = req; o.status = st;
    if (nsx_icmp_err_ipv4_dev_tuned(offs, offs, 1, req, arg, &cfg, &o, offs, 1 << 20, 0, &t) != NSX_EINVAL) return 5;
    if (nsx_icmp_req_frag_dev(st, 0, 1, req, arg, 0) != NSX_EINVAL) return 6;
    if (nsx_icmp_req_ttl_ipv4_dev(offs, offs, 1, mask, 256, req, arg, 0) != NSX_EINVAL) return 7;
    if (nsx_icmp_req_ttl_ipv6_dev(offs, offs, 1, 0, 1, req, arg, 0) != NSX_EINVAL) return 8;
    if (nsx_icmp_rx_ipv4_verify_dev(offs, offs, 1, 0, 0, 0, 0, 0) != NSX_EINVAL) return 9;
    if (nsx_icmp_rx_ipv6_verify_dev_tuned(0, offs, 1, mask, 0, 0, 0, &t) != NSX_EINVAL) return 10;
    if (nsx_icmp_echo_reply_ipv4_dev(st, offs, 1, mask, 256, mask, 0) != NSX_EINVAL) return 11;
    if (nsx_icmp_echo_reply_ipv6_dev(st, offs, 1, mask, 64, 0, 0) != NSX_EINVAL) return 12;
    return NSX_ICMP_NONE + NSX_ICMP_SENT + NSX_ICMP_QUIET + NSX_ICMP_BAD + NSX_ICMP_LIMITED - 10;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(nsx.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I", inc, "-L", libdir, "-lnsx_csum",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- validation
def _eout(null=()):
    return nsx.IcmpErrOut(*[None if k in null else 0x1000 for k, _, _ in nsx.ICMP_ERR_FIELDS])


def _err_call(ipver, tuned, n=100, out=None, **kw):
    a = dict(base=fake, offsets=fake, req=fake, arg=fake, cfg=nsx.IcmpErrCfg(ttl=64, max_out=10), work=fake,
             work_bytes=nsx.icmp_err_work_bytes(min(n, 1 << 20)))
    a.update(kw)
    o = _eout() if out is None else out
    args = [a["base"], a["offsets"], n, a["req"], a["arg"], None if a["cfg"] is None else ctypes.byref(a["cfg"]),
            None if o == "null" else ctypes.byref(o), a["work"], a["work_bytes"], None]
    if tuned:
        fn = getattr(nsx.lib(), f"nsx_icmp_err_ipv{ipver}_dev_tuned")
        return fn(*args, ctypes.byref(nsx.Tune(run_segs=16, blocks_per_cu=1)))
    return getattr(nsx.lib(), f"nsx_icmp_err_ipv{ipver}_dev")(*args)


@pytest.mark.parametrize("tuned", [False, True], ids=["plain", "tuned"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_err_calls_validate_before_any_device_work(ipver, tuned):
    """NULL pointers with n > 0, the always-required cfg / out / n_out / out_off / d_work, n >= 2^32 - 1, ttl > 255 and
    a workspace one byte short are NSX_EINVAL before anything else; d_arg may be NULL; a well-formed call on a host
    with no GPU is then NSX_ENODEV, n == 0 included."""
    need = nsx.icmp_err_work_bytes
    bad = [dict(base=None), dict(offsets=None), dict(req=None), dict(cfg=None), dict(work=None), dict(out="null"),
           dict(n=0xFFFFFFFF, work_bytes=1 << 62), dict(n=1 << 32, work_bytes=1 << 62),
           dict(cfg=nsx.IcmpErrCfg(ttl=256, max_out=1)), dict(cfg=nsx.IcmpErrCfg(ttl=0xFFFFFFFF, max_out=1)),
           dict(work_bytes=need(100) - 1), dict(work_bytes=0), dict(n=0, work_bytes=need(0) - 1),
           dict(n=0, cfg=None), dict(n=0, work=None), dict(n=0, out="null")]
    for kw in bad:
        assert _err_call(ipver, tuned, **kw) == E, kw
    for k, _, _ in nsx.ICMP_ERR_FIELDS:
        assert _err_call(ipver, tuned, out=_eout(null=(k,))) == E, k
    for k in ("n_out", "out_off"):
        assert _err_call(ipver, tuned, n=0, out=_eout(null=(k,))) == E, k
    if nsx.device_count() == 0:
        assert _err_call(ipver, tuned) == D
        assert _err_call(ipver, tuned, arg=None) == D
        assert _err_call(ipver, tuned, cfg=nsx.IcmpErrCfg(ttl=255, max_out=0)) == D
        assert _err_call(ipver, tuned, n=0, base=None, offsets=None, req=None, arg=None,
                         out=_eout(null=("out", "src_frame", "status"))) == D
        assert _err_call(ipver, tuned, n=0xFFFFFFFE, work_bytes=1 << 62) == D


def test_other_device_calls_validate_before_any_device_work():
    """The request helpers, the verify (plain and tuned) and the echo reply: a NULL array with n > 0, n >= 2^32 - 1
    and ttl / ttl_dec > 255 are NSX_EINVAL before anything else; every array may be NULL at n == 0, and the nullable
    outputs always; then NSX_ENODEV on a host with no GPU."""
    L = nsx.lib()
    tune = ctypes.byref(nsx.Tune(run_segs=7, blocks_per_cu=2))
    calls = {  # name: its arguments in order, the stream left out
        "nsx_icmp_req_frag_dev": "status mtu n req arg",
        "nsx_icmp_req_ttl_ipv4_dev": "base offsets n valid ttl req arg",
        "nsx_icmp_req_ttl_ipv6_dev": "base offsets n valid ttl req arg",
        "nsx_icmp_rx_ipv4_verify_dev": "base offsets n mask ip_raw icmp_raw type",
        "nsx_icmp_rx_ipv6_verify_dev": "base offsets n mask icmp_raw type",
        "nsx_icmp_echo_reply_ipv4_dev": "base offsets n valid ttl hit",
        "nsx_icmp_echo_reply_ipv6_dev": "base offsets n valid ttl hit",
    }
    nullable = {"ip_raw", "icmp_raw", "type"}
    for name, names in calls.items():
        names = names.split()
        for tuned in ((False, True) if "_rx_" in name else (False,)):
            fn = getattr(L, name + ("_tuned" if tuned else ""))

            def call(**kw):
                a = {k: fake for k in names}
                a.update(n=100, ttl=1)
                a.update(kw)
                return fn(*[a[k] for k in names], None, *([tune] if tuned else []))

            ptrs = [k for k in names if k not in ("n", "ttl")]
            for k in ptrs:
                if k not in nullable:
                    assert call(**{k: None}) == E, (name, k)
                elif nsx.device_count() == 0:
                    assert call(**{k: None}) == D, (name, k)
            assert call(n=0xFFFFFFFF) == E and call(n=1 << 32) == E
            if "ttl" in names:
                assert call(ttl=256) == E and call(ttl=0xFFFFFFFF) == E and call(n=0, ttl=256) == E
            if nsx.device_count() == 0:
                assert call() == D and call(n=0xFFFFFFFE) == D
                assert call(n=0, **{k: None for k in ptrs}) == D
                if "ttl" in names:
                    assert call(ttl=0) == D and call(ttl=255) == D


def test_err_work_bytes_is_monotone_and_sufficient():
    """Nondecreasing in n, strictly over these sizes; it holds a dword per frame, a pair of sums per 16 frames (the
    smallest scan block a tune can ask for) and the rounding of the caller's pointer; it refuses n >= 2^32 - 1 and a
    NULL out."""
    ns = (0, 1, 15, 16, 17, 255, 256, 257, 4096, 4097, 1 << 20, 0xFFFFFFFE)
    w = [nsx.icmp_err_work_bytes(n) for n in ns]
    assert all(b > a for a, b in zip(w, w[1:]))
    for n, a in zip(ns, w):
        assert 4 * n + 16 * ((n + 15) // 16 + 1) + 7 <= a <= 5 * n + 64, n
    c = ctypes.c_uint64(0)
    fn = nsx.lib().nsx_icmp_err_work_bytes
    assert fn(0xFFFFFFFF, ctypes.byref(c)) == E and fn(1 << 40, ctypes.byref(c)) == E and fn(5, None) == E
    assert fn(0xFFFFFFFE, ctypes.byref(c)) == OK
    with pytest.raises(nsx.NsxError) as e:
        nsx.icmp_err_work_bytes(0xFFFFFFFF)
    assert e.value.code == E


def test_binding_checks_extents_before_the_c_call():
    """Every given tensor's extent and dtype is checked before the C call (CPU tensors here: a well-formed call is then
    refused as not on a device)."""
    import torch
    n = 70
    offs = torch.arange(n + 1, dtype=torch.int64) * 60
    buf = torch.zeros(60 * n, dtype=torch.uint8)
    req = torch.zeros(n, dtype=torch.int32)
    words = torch.zeros(2, dtype=torch.int64)
    u16 = torch.zeros(n, dtype=torch.int16)
    need = nsx.icmp_err_work_bytes(n)
    assert nsx.icmp_err_out_bytes(4, n, 10, buf.numel()) == buf.numel() + 10 * 28
    assert nsx.icmp_err_out_bytes(4, n, 3, buf.numel()) == 3 * 576
    assert nsx.icmp_err_out_bytes(6, n, 1 << 40, buf.numel()) == buf.numel() + 48 * n
    for ipver, fn in ((4, nsx.icmp_err_ipv4_dev), (6, nsx.icmp_err_ipv6_dev)):
        src = A4 if ipver == 4 else A6
        cases = [(dict(offsets=offs.to(torch.int32)), "8-byte elements"), (dict(buf=buf.view(torch.int16)), "1-byte elements"),
                 (dict(req=None), "`req` are required"), (dict(req=req[:-1]), " req"),
                 (dict(req=req.to(torch.int64)), "4-byte elements"), (dict(arg=req[:-1]), " arg"),
                 (dict(src=src[:-1]), "address bytes"), (dict(ttl=-1), "unsigned"),
                 (dict(work=torch.zeros(need - 1, dtype=torch.uint8)), " work"), (dict(out={"bogus": buf}), "unknown output"),
                 (dict(out={"out_off": torch.zeros(n, dtype=torch.int64)}), " out_off"),
                 (dict(max_out=5, out={"src_frame": torch.zeros(4, dtype=torch.int32)}), " src_frame"),
                 (dict(out={"src_frame": torch.zeros(n, dtype=torch.int64)}), "4-byte elements"),
                 (dict(out={"status": torch.zeros(n - 1, dtype=torch.uint8)}), " status"),
                 (dict(out={"n_out": torch.zeros(1, dtype=torch.int32)}), "8-byte elements"), (dict(), "device")]
        for kw, msg in cases:
            args = dict(buf=buf, offsets=offs, req=req, src=src)
            args.update(kw)
            with pytest.raises(ValueError) as e:
                fn(**args)
            assert msg in str(e.value), (msg, str(e.value))
    for fn, extra in ((nsx.icmp_rx_ipv4_verify_dev, dict(ip_raw=u16[:-1])), (nsx.icmp_rx_ipv6_verify_dev, {})):
        for kw, msg in [(dict(mask=words[:1]), " mask"), (dict(mask=words.to(torch.int32)), "8-byte elements"),
                        (dict(icmp_raw=u16[:-1]), " icmp_raw"), (dict(type=u16[:-1]), " type"),
                        (dict(type=req), "2-byte elements"), (dict(), "device")] + \
                       ([(extra, " ip_raw")] if extra else []):
            with pytest.raises(ValueError) as e:
                fn(buf, offs, **kw)
            assert msg in str(e.value), (msg, str(e.value))
    for fn in (nsx.icmp_echo_reply_ipv4_dev, nsx.icmp_echo_reply_ipv6_dev):
        for kw, msg in [(dict(valid=None), "`valid` is required"), (dict(valid=words[:1]), " valid"),
                        (dict(hit=words[:1]), " hit"), (dict(hit=words.to(torch.int32)), "8-byte elements"),
                        (dict(ttl=-1), "ttl"), (dict(), "device")]:
            args = dict(valid=words)
            args.update(kw)
            with pytest.raises(ValueError) as e:
                fn(buf, offs, **args)
            assert msg in str(e.value), (msg, str(e.value))
    for fn in (nsx.icmp_req_ttl_ipv4_dev, nsx.icmp_req_ttl_ipv6_dev):
        for kw, msg in [(dict(valid=None), "are required"), (dict(valid=words[:1]), " valid"), (dict(req=req[:-1]), " req"),
                        (dict(arg=req[:-1]), " arg"), (dict(arg=u16), "4-byte elements"), (dict(ttl_dec=-1), "ttl_dec"),
                        (dict(), "device")]:
            args = dict(valid=words, ttl_dec=1, req=req, arg=req.clone())
            args.update(kw)
            with pytest.raises(ValueError) as e:
                fn(buf, offs, **args)
            assert msg in str(e.value), (msg, str(e.value))
    st = torch.zeros(n, dtype=torch.uint8)
    for kw, msg in [(dict(status=st[:-1]), " status"), (dict(mtu=req[:-1]), " mtu"), (dict(arg=req[:-1]), " arg"),
                    (dict(mtu=None), "are required"), (dict(req=req.to(torch.int64)), "4-byte elements"), (dict(), "device")]:
        args = dict(status=st, mtu=req.clone(), req=req, arg=req.clone())
        args.update(kw)
        with pytest.raises(ValueError) as e:
            nsx.icmp_req_frag_dev(**args)
        assert msg in str(e.value), (msg, str(e.value))


# ---------------------------------------------------------------- the model against known answers
def test_known_answers_by_hand():
    """RFC 792 echo with id 1, seq 1 and no data: 08 00 | cs | 00 01 00 01 sums to 0x0802, so the checksum is 0xF7FD;
    the reply's words sum to 0x0002: 0xFFFD. A message over a 21-byte frame ends in an odd byte, which is summed as
    the high byte of a word whose low byte is zero."""
    rq = M.echo4(A4, B4)
    assert rq[20:] == bytes.fromhex("0800f7fd00010001") and len(rq) == 28
    rp = M.echo_frame(rq, 64, 4)
    assert rp[20:] == bytes.fromhex("0000fffd00010001") and rp[12:16] == B4 and rp[16:20] == A4
    assert M.update(0xF7FD, 0x0800, 0x0000) == 0xFFFD
    f = M.ip4(17, B4, A4, b"\xab", ttl=1)  # 21 bytes
    assert len(f) == 21
    m = M.message(f, 11, 0, A4, 64, 7, 4)
    assert len(m) == 28 + 21 and m[:2] == b"\x45\xc0" and m[2:4] == (49).to_bytes(2, "big") and m[4:6] == b"\0\7"
    assert m[8:10] == b"\x40\x01" and m[12:16] == A4 and m[16:20] == B4 and m[28:] == f
    words = [int.from_bytes(m[k:k + 2], "big") for k in range(20, 48, 2) if k != 22] + [0xAB00]
    s = sum(words)
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    assert int.from_bytes(m[22:24], "big") == ~s & 0xFFFF
    assert M.raw(m[20:]) == 0xFFFF and M.raw(m[:20]) == 0xFFFF
    # the fold is the NAT comment's, value for value
    assert all(M.fold(x) == _nat.fold(x) for x in (0, 1, 0xFFFE, 0xFFFF, 0x10000, 0x1FFFE, 0x1FFFF, 0x2FFFD))


# ---------------------------------------------------------------- one hand case per status rule
def _status(f, r, ipver, max_out=9):
    buf, offs = M.pack([f], lead=1)
    return int(M.err(buf, offs, [r], None, A4 if ipver == 4 else A6, 64, 0, max_out, ipver)["status"][0])


def test_every_status_rule_ipv4():
    udp = M.ip4(17, B4, A4, bytes(12))
    assert _status(udp, 0, 4) == M.NONE                                  # no request
    assert _status(udp, 11, 4) == M.SENT and _status(udp, 3 | 4 << 8, 4) == M.SENT and _status(udp, 12, 4) == M.SENT
    assert _status(udp, 11, 4, max_out=0) == M.LIMITED                   # RFC 1812 §4.3.2.8: the rate cap
    for r in (5, 8, 0, 255, 11 | 1 << 16, 3 | 1 << 31):                  # redirect, echo, unknown types; high bits
        assert _status(udp, r, 4) == (M.BAD if r else M.NONE), r
    for g in (udp[:19], bytes([0x65]) + udp[1:], bytes([0x44]) + udp[1:], bytes([0x4F]) + udp[1:], udp + b"\0",
              udp[:-1], b""):                                           # RFC 791 §3.1: the header does not parse
        assert _status(g, 11, 4) == M.BAD
    frag = lambda w: M.ip4(17, B4, A4, bytes(16), flags_off=w)  # noqa: E731
    assert _status(frag(0x2000), 11, 4) == M.SENT                        # RFC 1122 §3.2.2: the first fragment is answered
    assert _status(frag(0x0001), 11, 4) == M.QUIET and _status(frag(0x3FFF), 11, 4) == M.QUIET  # a non-initial fragment
    for src in (bytes(4), bytes([224, 0, 0, 1]), bytes([255] * 4), bytes([240, 1, 2, 3])):  # RFC 1812 §4.3.2.7
        assert _status(M.ip4(17, src, A4, bytes(8)), 11, 4) == M.QUIET
    assert _status(M.ip4(17, bytes([223, 255, 255, 255]), A4, bytes(8)), 11, 4) == M.SENT
    for dst in (bytes([224, 0, 0, 5]), bytes([255] * 4)):                # RFC 1122 §3.2.2: multicast / broadcast dst
        assert _status(M.ip4(17, B4, dst, bytes(8)), 11, 4) == M.QUIET
    for t in range(0, 20):                                               # RFC 1122 §3.2.2: no error about an error
        f = M.ip4(1, B4, A4, M.icmp4(t, 0, bytes(4)))
        assert _status(f, 11, 4) == (M.SENT if t in M.QUERY4 else M.QUIET), t
    assert _status(M.ip4(1, B4, A4, M.icmp4(40, 0, bytes(4))), 11, 4) == M.QUIET
    assert _status(M.ip4(1, B4, A4, b""), 11, 4) == M.QUIET              # protocol 1 and no type byte
    assert _status(M.ip4(1, B4, A4, b"\x08"), 11, 4) == M.SENT           # the type byte alone is enough
    # the first rule that matches decides: a bad request over a frame that would be QUIET is BAD
    assert _status(frag(0x0001), 5, 4) == M.BAD


def test_every_status_rule_ipv6():
    udp = M.ip6(17, B6, A6, bytes(12))
    assert _status(udp, 0, 6) == M.NONE
    for r in (1, 2, 3, 4, 4 | 2 << 8, 1 | 255 << 8):
        assert _status(udp, r, 6) == M.SENT
    assert _status(udp, 3, 6, max_out=0) == M.LIMITED                    # RFC 4443 §2.4(f)
    for r in (5, 11, 128, 137, 3 | 1 << 16):
        assert _status(udp, r, 6) == M.BAD
    for g in (udp[:39], bytes([0x40]) + udp[1:], udp + b"\0", udp[:-1]):
        assert _status(g, 3, 6) == M.BAD
    mc = bytes([0xFF, 2] + [0] * 13 + [1])
    assert _status(M.ip6(17, bytes(16), A6, bytes(8)), 3, 6) == M.QUIET  # RFC 4443 §2.4(e.6): the unspecified address
    assert _status(M.ip6(17, mc, A6, bytes(8)), 3, 6) == M.QUIET         # (e.6): a multicast source
    to_mc = M.ip6(17, B6, mc, bytes(8))
    assert _status(to_mc, 3, 6) == M.QUIET and _status(to_mc, 1, 6) == M.QUIET  # (e.3)
    assert _status(to_mc, 2, 6) == M.SENT and _status(to_mc, 4 | 2 << 8, 6) == M.SENT  # (e.3)'s two exceptions
    assert _status(to_mc, 4 | 1 << 8, 6) == M.QUIET
    for t, want in ((1, M.QUIET), (4, M.QUIET), (127, M.QUIET), (128, M.SENT), (129, M.SENT), (135, M.SENT),
                    (137, M.QUIET), (138, M.SENT)):                      # (e.1) an error, (e.2) a redirect
        assert _status(M.ip6(58, B6, A6, M.icmp6(t, 0, bytes(4), b"", B6, A6)), 3, 6) == want, t
    assert _status(M.ip6(58, B6, A6, b""), 3, 6) == M.QUIET              # Next Header 58 and no type byte
    assert _status(M.ip6(58, B6, A6, b"\x80"), 3, 6) == M.SENT
    # extension headers are not walked: an ICMPv6 error behind a hop-by-hop header is answered
    hbh = bytes([58, 0, 1, 4, 0, 0, 0, 0]) + M.icmp6(1, 0, bytes(4), b"", B6, A6)
    assert _status(M.ip6(0, B6, A6, hbh), 3, 6) == M.SENT


# ---------------------------------------------------------------- the model against itself
def _mixed_frames(rng, ipver, n):
    fr = []
    edge = M.QUOTE[ipver] - (20 if ipver == 4 else 40)  # the payload whose frame is exactly the longest quote
    lens = [0, 1, 5, 8, 9, 100, edge - 1, edge, edge + 1, 1400]
    for i in range(n):
        L = lens[i % len(lens)]
        pay = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        src = bytes(rng.integers(1, 200, 4 if ipver == 4 else 16, dtype=np.uint8))
        fr.append(M.ip4(17, src, A4, pay) if ipver == 4 else M.ip6(17, src, A6, pay))
    return fr


@pytest.mark.parametrize("ipver", [4, 6])
def test_every_generated_message_verifies_and_quotes_its_frame(ipver):
    """Quotes either side of the cap (547 / 548 / 549, 1231 / 1232 / 1233 bytes) and odd ones: every message passes
    the model's verify with the request's type word, carries the argument in bytes 4-7 and quotes min(len, Q) bytes;
    a message about a message is QUIET; the worst-case extent holds."""
    rng = np.random.default_rng(0x1C30 + ipver)
    fr = _mixed_frames(rng, ipver, 60)
    lens = {len(f) for f in fr}
    Q = M.QUOTE[ipver]
    assert {Q - 1, Q, Q + 1} <= lens
    types = M.ALLOWED[ipver]
    req = np.array([int(types[i % len(types)]) | (i % 5) << 8 for i in range(60)], np.uint32)
    arg = rng.integers(0, 1 << 32, 60, dtype=np.uint64).astype(np.uint32)
    src = A4 if ipver == 4 else A6
    buf, offs = M.pack(fr, lead=3)
    r = M.err(buf, offs, req, arg, src, 200, 0xFFFE, 1 << 40, ipver)
    assert r["n_out"] == 60 and (r["status"] == M.SENT).all() and r["src_frame"].tolist() == list(range(60))
    assert int(r["out_off"][-1]) == M.out_bytes_worst(fr, 60, ipver) == r["out"].size
    mbuf, moffs = M.pack(r["msgs"], lead=1)
    v = M.verify(mbuf, moffs, ipver)
    assert v["ok"].all()
    assert v["type"].tolist() == [((int(q) & 0xFF) << 8) | (int(q) >> 8) for q in req]
    h = M.HDR[ipver]
    for i, m in enumerate(r["msgs"]):
        assert m[h:] == fr[i][:Q] and m[h - 4:h] == int(arg[i]).to_bytes(4, "big")
        if ipver == 4:
            assert int.from_bytes(m[4:6], "big") == (0xFFFE + i) & 0xFFFF and m[8] == 200 and m[16:20] == fr[i][12:16]
        else:
            assert m[7] == 200 and m[24:40] == fr[i][8:24] and m[8:24] == A6
    again = M.err(mbuf, moffs, req, None, src, 64, 0, 1 << 40, ipver)
    assert (again["status"] == M.QUIET).all() and again["n_out"] == 0 and again["out_off"].tolist() == [0]
    capped = M.err(buf, offs, req, arg, src, 200, 0, 7, ipver)
    assert capped["n_out"] == 7 and capped["status"].tolist() == [M.SENT] * 7 + [M.LIMITED] * 53
    assert capped["msgs"] == [M.message(fr[i], int(req[i]), int(arg[i]), src, 200, i, ipver) for i in range(7)]


@pytest.mark.parametrize("ipver", [4, 6])
def test_echo_reply_then_verify_equals_a_rebuild_from_scratch(ipver):
    """Requests of every payload length 0..40 and 1471 / 1472, IPv4 with options too: the reply verifies and is byte
    for byte the reply built from scratch; a wrong checksum stays wrong by the same one's-complement difference;
    replies, other types, code 1, a multicast dst, fragments and a clear valid bit are left alone."""
    rng = np.random.default_rng(0x1C40 + ipver)
    fr = []
    for L in list(range(41)) + [1471, 1472]:
        data = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        if ipver == 4:
            opt = rng.integers(0, 256, 4 * (L % 11), dtype=np.uint8).tobytes()
            fr.append(M.echo4(B4, A4, ident=int(rng.integers(1 << 16)), seq=L, data=data, ttl=int(rng.integers(1, 256)),
                              options=opt, ip_ident=L * 7))
        else:
            fr.append(M.echo6(B6, A6, ident=int(rng.integers(1 << 16)), seq=L, data=data, hop=int(rng.integers(1, 256)),
                              flow=L * 1000))
    buf, offs = M.pack(fr, lead=1)
    assert M.verify(buf, offs, ipver)["ok"].all()
    out, hit = M.echo(buf, offs, np.ones(len(fr), bool), 77, ipver)
    assert hit.all()
    v = M.verify(out, offs, ipver)
    assert v["ok"].all() and (v["type"] == (0 if ipver == 4 else 129 << 8)).all()
    assert M.frames_of(out, offs) == [M.rebuilt_reply(f, 77, ipver) for f in fr]
    same = np.ones(buf.size, bool)
    same[int(offs[0]):int(offs[-1])] = False
    assert np.array_equal(out[same], buf[same])
    # wrong sums: the ICMP checksum, and on IPv4 the header checksum
    ihl = lambda f: (f[0] & 15) * 4 if ipver == 4 else 40  # noqa: E731
    for at_of in ((lambda f: ihl(f) + 2),) + (((lambda f: 10),) if ipver == 4 else ()):
        for f in fr[:12]:
            at = at_of(f)
            g = bytearray(f)
            g[at] ^= 0x41
            g[at + 1] ^= 0xFF
            r, good = M.echo_frame(bytes(g), 77, ipver), M.echo_frame(f, 77, ipver)
            be = lambda b: int.from_bytes(b[at:at + 2], "big")  # noqa: E731
            assert r[:at] == good[:at] and r[at + 2:] == good[at + 2:]
            assert (be(r) - be(good)) % 0xFFFF == (be(g) - be(f)) % 0xFFFF != 0
    mc4, mc6 = bytes([224, 0, 0, 1]), bytes([0xFF, 2] + [0] * 13 + [1])
    if ipver == 4:
        alone = [M.echo4(B4, A4, reply=True), M.ip4(1, B4, A4, M.icmp4(8, 1, bytes(4))), M.echo4(B4, mc4),
                 M.ip4(1, B4, A4, M.icmp4(13, 0, bytes(4), bytes(12))), M.ip4(1, B4, A4, M.icmp4(8, 0, bytes(4)), flags_off=0x2000),
                 M.ip4(17, B4, A4, M.icmp4(8, 0, bytes(4))), M.echo4(B4, A4)[:-1]]
    else:
        alone = [M.echo6(B6, A6, reply=True), M.ip6(58, B6, A6, M.icmp6(128, 1, bytes(4), b"", B6, A6)), M.echo6(B6, mc6),
                 M.ip6(58, B6, A6, M.icmp6(135, 0, bytes(4), bytes(16), B6, A6)), M.ip6(17, B6, A6, bytes(8)),
                 M.echo6(B6, A6)[:-1]]
    abuf, aoffs = M.pack(alone + [fr[3]], lead=2)
    valid = np.ones(len(alone) + 1, bool)
    valid[-1] = False
    out, hit = M.echo(abuf, aoffs, valid, 9, ipver)
    assert not hit.any() and np.array_equal(out, abuf)


def test_frag_status_goes_through_req_frag_into_the_error_model():
    """tests/_frag.py's status 2 (NSX_FRAG_DF) -> req_frag -> the error model: a "fragmentation needed" whose next-hop
    MTU lands in ICMP bytes 6-7 (RFC 1191), composed with a TTL request on the same arrays."""
    rng = np.random.default_rng(0x1C50)
    frames = _frag.udp_frames(rng, [100, 1472, 1473, 3000], df=True) + _frag.udp_frames(rng, [2000], df=False)
    mtu = np.array([1500, 1500, 1500, 576 | 1 << 16, 1500], np.uint32)
    _, status = _frag.frag_frames(frames, [int(m) & 0xFFFF for m in mtu])
    assert status.tolist() == [_frag.PASS, _frag.PASS, _frag.DF, _frag.DF, _frag.CUT] and _frag.DF == M.FRAG_DF
    buf, offs = M.pack(frames, lead=1)
    req, arg = M.req_frag(status, mtu, np.zeros(5, np.uint32), np.full(5, 0xDEAD, np.uint32))
    assert req.tolist() == [0, 0, 0x0403, 0x0403, 0] and arg.tolist() == [0xDEAD, 0xDEAD, 1500, 576, 0xDEAD]
    valid = np.array([True, False, True, True, True])
    frames[0] = frames[0][:8] + b"\x01" + frames[0][9:]  # TTL 1 (the header checksum is not looked at here)
    buf, offs = M.pack(frames, lead=1)
    req, arg = M.req_ttl(buf, offs, valid, 1, req, arg, 4)
    assert req.tolist() == [11, 0, 0x0403, 0x0403, 0] and arg.tolist() == [0, 0xDEAD, 1500, 576, 0xDEAD]
    r = M.err(buf, offs, req, arg, A4, 64, 0, 10, 4)
    assert r["status"].tolist() == [M.SENT, M.NONE, M.SENT, M.SENT, M.NONE] and r["src_frame"].tolist() == [0, 2, 3]
    assert [m[20:22] for m in r["msgs"]] == [b"\x0b\0", b"\x03\x04", b"\x03\x04"]
    assert [int.from_bytes(m[26:28], "big") for m in r["msgs"]] == [0, 1500, 576] and all(m[24:26] == b"\0\0" for m in r["msgs"])
    mbuf, moffs = M.pack(r["msgs"])
    assert M.verify(mbuf, moffs, 4)["type"].tolist() == [0x0B00, 0x0304, 0x0304]
