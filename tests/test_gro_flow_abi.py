"""Flow-keyed receive coalescing's boundary (nsx_gro_flow_*), on any host: the symbols, every NSX_EINVAL before
NSX_ENODEV, the workspace size, the binding's extent checks, and the numpy restatement tests/_gro_flow.py held to what
already exists — tests/_gro.py on one connection, segmentation offload's expansion (tests/_tso.py) on interleaved
ones. The GPU tests (tests/test_gpu_gro_flow.py) compare the kernels against tests/_gro_flow.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nsx
import _gro
import _gro_flow as FL
import _tso

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_CALLS = ("nsx_gro_flow_ipv4_tcp_dev", "nsx_gro_flow_ipv6_tcp_dev")
fake = ctypes.c_void_p(0x1000)


# ---------------------------------------------------------------- symbols
def test_gro_flow_symbols_are_declared_and_exported(tmp_path):
    """nsx_csum.h declares nsx_gro_flow_work_bytes and the two device calls, nsx_gro_tune.h their _tuned twins; the
    library exports all five; the ABI version stays 2; the header says what the calls do and nsx_gro_* points to
    them; a plain C caller compiles against them and gets the documented codes from the validation."""
    inc = os.path.join(ROOT, "include")
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)  # noqa: E731
    decl = r"^int\s+(nsx_gro_flow_[a-z_0-9]+)\("
    text = open(os.path.join(inc, "nsx_csum.h")).read()
    plain = set(re.findall(decl, strip(text), flags=re.M))
    tuned = set(re.findall(decl, strip(open(os.path.join(inc, "nsx_gro_tune.h")).read()), flags=re.M))
    assert plain == set(DEV_CALLS) | {"nsx_gro_flow_work_bytes"}
    assert tuned == {f + "_tuned" for f in DEV_CALLS}
    out = subprocess.run(["nm", "-D", "--defined-only", nsx.LIB_PATH], capture_output=True, text=True).stdout
    assert plain | tuned <= set(re.findall(r" T (nsx_\w+)", out))
    assert nsx.abi_version() == 2
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for word in ("nsx_gro_flow_ipv4_tcp_dev / nsx_gro_flow_ipv6_tcp_dev below coalesce per connection",
                 "0x811C9DC5", "0x01000193", "equal keys keep arrival order", "first_frame[s] is a position",
                 "frame_seg[d_order[p]] = frame_seg'[p]", "does not write d_order", "never makes a wrong merge"):
        assert word in flat, word
    assert "keys per tile of the radix sort in units of 256" in \
        re.sub(r"\s*\n \*\s*", " ", open(os.path.join(inc, "nsx_gro_tune.h")).read())
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include "nsx_tune.h"
int main(void) {
    nsx_gro_out o = {0};
    nsx_tune t = {0};
    uint64_t need = 0, plain = 0, offs[1] = {0}, mask[1] = {0};
    uint32_t order[1];
    if (nsx_gro_flow_work_bytes(1000, &need) != NSX_OK || nsx_gro_work_bytes(1000, &plain) != NSX_OK) return 1;
    if (need < plain + 16 * 1000) return 2;
    if (nsx_gro_flow_work_bytes(0xFFFFFFFFull, &need) != NSX_EINVAL || nsx_gro_flow_work_bytes(1, 0) != NSX_EINVAL)
        return 3;
    if (nsx_gro_flow_ipv4_tcp_dev(offs, offs, 0, mask, order, &o, offs, 1 << 20, 0) != NSX_EINVAL) return 4;
    if (nsx_gro_flow_ipv6_tcp_dev_tuned(offs, offs, 0, mask, order, 0, offs, 1 << 20, 0, &t) != NSX_EINVAL) return 5;
    return 0;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(nsx.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I", inc, "-L", libdir, "-lnsx_csum",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- validation
def _out(null=()):
    return nsx.GroOut(*[None if k in null else 0x1000 for k, _, _ in nsx.GRO_FIELDS])


def _call(name, n=100, tuned=False, out=None, **kw):
    a = dict(base=fake, offsets=fake, valid=fake, order=fake, work=fake,
             work_bytes=nsx.gro_flow_work_bytes(min(n, 1 << 20)))
    a.update(kw)
    o = _out() if out is None else out
    args = [a["base"], a["offsets"], n, a["valid"], a["order"], None if o == "null" else ctypes.byref(o), a["work"],
            a["work_bytes"], None]
    if tuned:
        return getattr(nsx.lib(), name + "_tuned")(*args, ctypes.byref(nsx.Tune(rows=1, run_segs=16)))
    return getattr(nsx.lib(), name)(*args)


def test_gro_flow_device_calls_validate_before_any_device_work():
    """NULL pointers (d_order with n > 0 among them), every NULL member of nsx_gro_out, n >= 2^32 - 1 and a workspace
    one byte short — nsx_gro_work_bytes(n) is too little — are NSX_EINVAL before anything else; a well-formed call
    on a host with no GPU is then NSX_ENODEV, n == 0 (where d_order may be NULL) included."""
    E = nsx.NSX_EINVAL
    assert nsx.gro_work_bytes(100) < nsx.gro_flow_work_bytes(100)
    for name in DEV_CALLS:
        for tuned in (False, True):
            for kw in (dict(base=None), dict(offsets=None), dict(valid=None), dict(order=None), dict(work=None),
                       dict(out="null"), dict(n=0xFFFFFFFF, work_bytes=1 << 62), dict(n=1 << 32, work_bytes=1 << 62),
                       dict(work_bytes=nsx.gro_flow_work_bytes(100) - 1), dict(work_bytes=nsx.gro_work_bytes(100)),
                       dict(work_bytes=0), dict(n=0, work_bytes=nsx.gro_flow_work_bytes(0) - 1),
                       dict(n=0, offsets=None)):
                assert _call(name, tuned=tuned, **kw) == E, kw
            for k, _, _ in nsx.GRO_FIELDS:
                assert _call(name, tuned=tuned, out=_out(null=(k,))) == E, k
            if nsx.device_count() == 0:
                assert _call(name, tuned=tuned) == nsx.NSX_ENODEV
                assert _call(name, tuned=tuned, n=0, base=None, valid=None, order=None) == nsx.NSX_ENODEV
                assert _call(name, tuned=tuned, n=0xFFFFFFFE, work_bytes=1 << 62) == nsx.NSX_ENODEV


def test_gro_flow_work_bytes():
    """Monotone in n, at least nsx_gro_work_bytes(n) plus the four key / index buffers and the digit table of the
    smallest tile (rows = 1: 256 counters per 256 keys), n = 0 included; refuses n >= 2^32 - 1."""
    ns = (0, 1, 255, 256, 257, 4096, 4097, 1 << 20, 0xFFFFFFFE)
    w = [nsx.gro_flow_work_bytes(n) for n in ns]
    assert all(b > a for a, b in zip(w, w[1:]))
    for n, b in zip(ns, w):
        assert b >= nsx.gro_work_bytes(n) + 16 * n + 4 * 256 * ((n + 255) // 256), n
        assert b <= nsx.gro_work_bytes(n) + 20 * n + 2048, n
    assert w[0] >= nsx.gro_work_bytes(0) >= 8
    with pytest.raises(nsx.NsxError) as e:
        nsx.gro_flow_work_bytes(0xFFFFFFFF)
    assert e.value.code == nsx.NSX_EINVAL


def test_gro_flow_binding_checks_extents_before_the_c_call():
    """As gro_ipv4_tcp_dev's: every given tensor is checked before the C call (CPU tensors here: a well-formed call
    is then refused as not on a device) — and `order` and the larger workspace with them."""
    import torch
    n = 70
    offs = torch.arange(n + 1, dtype=torch.int64) * 60
    buf = torch.zeros(60 * n, dtype=torch.uint8)
    valid = torch.zeros(2, dtype=torch.int64)
    for ipver, fn in ((4, nsx.gro_flow_ipv4_tcp_dev), (6, nsx.gro_flow_ipv6_tcp_dev)):
        alen = 4 if ipver == 4 else 16
        cases = [(dict(valid=valid[:1]), " valid"), (dict(valid=None), "`valid` is required"),
                 (dict(valid=torch.zeros(4, dtype=torch.int32)), "8-byte elements"),
                 (dict(order=torch.zeros(n - 1, dtype=torch.int32)), " order"),
                 (dict(order=torch.zeros(n, dtype=torch.int64)), "4-byte elements"),
                 (dict(work=torch.zeros(nsx.gro_flow_work_bytes(n) - 1, dtype=torch.uint8)), " work"),
                 (dict(work=torch.zeros(nsx.gro_work_bytes(n), dtype=torch.uint8)), " work"),
                 (dict(out={"bogus": buf}), "unknown output"),
                 (dict(out={"src": torch.zeros(alen * n - 1, dtype=torch.uint8)}), " src"),
                 (dict(out={"frame_seg": torch.zeros(n - 1, dtype=torch.int32)}), " frame_seg:")]
        cases.append((dict(), "device"))
        for kw, msg in cases:
            args = dict(buf=buf, offsets=offs, valid=valid)
            args.update(kw)
            with pytest.raises(ValueError) as e:
                fn(**args)
            assert msg in str(e.value), (msg, str(e.value))
            assert f"gro_flow_ipv{ipver}_tcp_dev" in str(e.value) or msg == "device"


# ---------------------------------------------------------------- the model, held to what exists
def test_key_definition():
    """The key by hand for one IPv4 frame; a non-member's is 0xFFFFFFFF; the two helpers invert the last step."""
    rng = np.random.default_rng(0x5F0)
    for ipver in (4, 6):
        f = _gro.case_frames(_gro.flow_case(rng, ipver, [100]))[0]
        ihl = 20 if ipver == 4 else 40
        h = 0x811C9DC5
        raw = (f[12:20] if ipver == 4 else f[8:40]) + f[ihl:ihl + 4]
        for k in range(0, len(raw), 4):
            h = ((h ^ int.from_bytes(raw[k:k + 4], "little")) * 0x01000193) % (1 << 32)
        assert FL.key(f, ipver) == h != FL.NO_FLOW
        bad = bytearray(f)
        bad[ihl + 12] = 0x40  # doff 4
        assert FL.key(bytes(bad), ipver) == FL.NO_FLOW and FL.key(f[:-1], ipver) == FL.NO_FLOW
        g = _gro.case_frames(_gro.flow_case(rng, ipver, [100]))[0]
        assert FL.key(g, ipver) != h
        g2 = FL.with_ports(g, ipver, FL.colliding_ports(f, g, ipver))
        assert FL.key(g2, ipver) == h and g2[:ihl] == g[:ihl] and _gro.parse(g2, ipver) is not None
        for k in (0, 1, 0xFFFFFFFF, 0x12345678):
            assert FL.key(FL.with_ports(f, ipver, FL.ports_for_key(FL.state(f, ipver), k)), ipver) == k


@pytest.mark.parametrize("ipver", [4, 6])
def test_model_on_one_connection_is_the_adjacency_model(ipver):
    """One connection: every key equal, `order` the identity, every array tests/_gro.gro's."""
    rng = np.random.default_rng(0x5F1 + ipver)
    buf, offs = _gro.pack(_gro.case_frames(_gro.flow_case(rng, ipver, [700, 700, 300, 700, 700, 700, 5])), lead=1)
    valid = np.ones(7, bool)
    want = _gro.gro(buf, offs, valid, ipver)
    got = FL.gro_flow(buf, offs, valid, ipver)
    assert got["order"].tolist() == list(range(7)) and want["n_super"] == 2
    for k, v in want.items():
        assert np.array_equal(got[k], v), k


@pytest.mark.parametrize("opt", [False, True], ids=["noopt", "opt"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_model_on_five_interleaved_connections(ipver, opt):
    """5 connections x 4 frames round-robin, one frame invalid: 19 super-segments by adjacency, 6 per connection;
    the non-member is last in `order`; every connection's frames are consecutive and in arrival order; and expanding
    the output with segmentation offload's model reproduces frame order[p] at position p."""
    buf, offs, valid = FL.five_by_four(ipver, opt=b"\x02\x04\x05\xb4" if opt else b"", lead=3)
    n = offs.size - 1
    assert n == 20
    assert _gro.gro(buf, offs, valid, ipver)["n_super"] == 19
    out = FL.gro_flow(buf, offs, valid, ipver)
    od = out["order"]
    assert out["n_super"] == 6 and sorted(out["frame_cnt"].tolist()) == [1, 2, 4, 4, 4, 4]
    assert od[-1] == FL.INVALID and sorted(od.tolist()) == list(range(n))
    assert out["frame_seg"][FL.INVALID] == _gro.NONE
    members = od[:-1]
    conn = members % 5  # round-robin: frame i is of connection i % 5
    runs = [list(members[conn == c]) for c in range(5)]
    assert all(r == sorted(r) for r in runs)
    assert (np.diff(conn) != 0).sum() == 4  # five blocks
    for s in range(6):  # first_frame is a position; frame_seg is by original frame
        f0, cnt = int(out["first_frame"][s]), int(out["frame_cnt"][s])
        assert (out["frame_seg"][od[f0:f0 + cnt]] == s).all()
    b = _gro.as_batch(out, ipver)
    buf2, _, c2 = _tso.expected(b)
    body, offs2 = _gro.dense(buf2, b.off, c2.flen)
    assert offs2.size - 1 == 19
    for p in range(19):
        f = int(od[p])
        assert body[int(offs2[p]):int(offs2[p + 1])].tobytes() == buf[int(offs[f]):int(offs[f + 1])].tobytes(), p
