"""UDP receive coalescing's boundary (nsx_ugro_*), on any host: the symbols, every NSX_EINVAL before NSX_ENODEV, the
workspace sizes, the binding's extent checks, and the numpy restatement tests/_ugro.py held to what already exists —
UDP segmentation offload's expansion and the receive verify of tests/_udp.py. The GPU tests (tests/test_gpu_ugro.py,
tests/test_gpu_ugro_fuzz.py) compare the kernels against tests/_ugro.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nsx
import _gro_flow as FL
import _udp
import _ugro as UG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_CALLS = ("nsx_ugro_ipv4_dev", "nsx_ugro_ipv6_dev")
FLOW_CALLS = ("nsx_ugro_flow_ipv4_dev", "nsx_ugro_flow_ipv6_dev")
DEV_CALLS = PLAIN_CALLS + FLOW_CALLS
SIZE_CALLS = ("nsx_ugro_work_bytes", "nsx_ugro_flow_work_bytes")
fake = ctypes.c_void_p(0x1000)
E, D = nsx.NSX_EINVAL, nsx.NSX_ENODEV


# ---------------------------------------------------------------- symbols
def test_ugro_symbols_are_declared_and_exported(tmp_path):
    """nsx_csum.h declares exactly the six calls and nsx_ugro_tune.h exactly the four _tuned twins; that header brings
    nsx_tune.h in and no other tune header names the calls; the library exports all ten; no nsx_udp_* or nsx_gro_*
    name is added; the ABI version stays 2; the header states the contract; a plain C caller compiles with -Wall
    -Werror and gets the documented codes."""
    inc = os.path.join(ROOT, "include")
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)  # noqa: E731
    decl = r"^int\s+(nsx_ugro_[a-z_0-9]+)\("
    text = open(os.path.join(inc, "nsx_csum.h")).read()
    assert set(re.findall(decl, strip(text), flags=re.M)) == set(DEV_CALLS) | set(SIZE_CALLS)
    tune = open(os.path.join(inc, "nsx_ugro_tune.h")).read()
    assert set(re.findall(decl, strip(tune), flags=re.M)) == {c + "_tuned" for c in DEV_CALLS}
    assert '#include "nsx_tune.h"' in tune
    for h in ("nsx_tune.h", "nsx_tx_tune.h", "nsx_gro_tune.h", "nsx_udp_tune.h"):
        assert "nsx_ugro_" not in open(os.path.join(inc, h)).read(), h
    out = subprocess.run(["nm", "-D", "--defined-only", nsx.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (nsx_\w+)", out))
    assert {s for s in exported if s.startswith("nsx_ugro_")} == \
        set(DEV_CALLS) | set(SIZE_CALLS) | {c + "_tuned" for c in DEV_CALLS}
    # the closed sets of the UDP passes and of TCP receive coalescing are what they were
    assert len([s for s in exported if s.startswith("nsx_udp_")]) == 14
    assert len([s for s in exported if s.startswith("nsx_gro_")]) == 10
    assert nsx.abi_version() == 2 and "NSX_ABI_VERSION 2 " in text
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for word in ("UDP receive coalescing (Linux UDP_GRO)", "U == P, no padding past the UDP length",
                 "its UDP checksum field is not 0", "udp_gro_receive_segment", "both UDP ports are equal",
                 "join(i) is the three-frame window of nsx_gro_*, word for word",
                 "no 64-datagram cap and no 64 KiB cap", "UDP_GRO_CNT_MAX", "gso[s] = max(pay_f, 1)",
                 "then the dword holding the two UDP ports", "at most the IP header and the 8 UDP header bytes",
                 "nsx_ugro_flow_work_bytes(n) >= nsx_ugro_work_bytes(n) for every tune setting",
                 "rebuild every member frame byte for byte, the UDP checksum included",
                 "0xFFFF where the field-zero raw sum is 0xFFFF", "does not write d_order",
                 "frames may lie past 2^32 in d_base", "receive coalescing is nsx_ugro_* below",
                 "the NAT rewrite stays TCP"):
        assert word in flat, word
    flat_tune = re.sub(r"\s*\n \*\s*", " ", tune)
    assert "keys per tile of the radix sort in units of 256" in flat_tune and "clamped to 16..65536" in flat_tune
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include "nsx_csum.h"
#include "nsx_ugro_tune.h"
int main(void) {
    nsx_ugro_out o = {0};
    nsx_tune t = {0};
    uint64_t need = 0, plain = 0, offs[1] = {0}, mask[1] = {0};
    uint32_t order[1];
    if (nsx_ugro_flow_work_bytes(1000, &need) != NSX_OK || nsx_ugro_work_bytes(1000, &plain) != NSX_OK) return 1;
    if (plain < 16 * 1000 || need < plain + 16 * 1000) return 2;
    if (nsx_ugro_flow_work_bytes(0xFFFFFFFFull, &need) != NSX_EINVAL || nsx_ugro_flow_work_bytes(1, 0) != NSX_EINVAL)
        return 3;
    if (nsx_ugro_work_bytes(0xFFFFFFFFull, &need) != NSX_EINVAL || nsx_ugro_work_bytes(1, 0) != NSX_EINVAL) return 4;
    if (nsx_ugro_ipv4_dev(offs, offs, 0, mask, &o, offs, 1 << 20, 0) != NSX_EINVAL) return 5;
    if (nsx_ugro_ipv6_dev_tuned(offs, offs, 0, mask, 0, offs, 1 << 20, 0, &t) != NSX_EINVAL) return 6;
    if (nsx_ugro_flow_ipv4_dev(offs, offs, 0, mask, order, &o, offs, 1 << 20, 0) != NSX_EINVAL) return 7;
    if (nsx_ugro_flow_ipv6_dev_tuned(offs, offs, 0, mask, order, 0, offs, 1 << 20, 0, &t) != NSX_EINVAL) return 8;
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
    return nsx.UgroOut(*[None if k in null else 0x1000 for k, _, _ in nsx.UGRO_FIELDS])


def _need(name, n):
    return nsx.ugro_flow_work_bytes(n) if "_flow_" in name else nsx.ugro_work_bytes(n)


def _call(name, n=100, tuned=False, out=None, **kw):
    flow = "_flow_" in name
    a = dict(base=fake, offsets=fake, valid=fake, order=fake, work=fake, work_bytes=_need(name, min(n, 1 << 20)))
    a.update(kw)
    o = _out() if out is None else out
    args = [a["base"], a["offsets"], n, a["valid"]] + ([a["order"]] if flow else []) + \
        [None if o == "null" else ctypes.byref(o), a["work"], a["work_bytes"], None]
    if tuned:
        return getattr(nsx.lib(), name + "_tuned")(*args, ctypes.byref(nsx.Tune(rows=1, run_segs=16, blocks_per_cu=1)))
    return getattr(nsx.lib(), name)(*args)


@pytest.mark.parametrize("tuned", [False, True], ids=["plain", "tuned"])
@pytest.mark.parametrize("name", DEV_CALLS)
def test_ugro_device_calls_validate_before_any_device_work(name, tuned):
    """NULL pointers (d_order with n > 0 among them, for the flow-keyed form), every NULL member of nsx_ugro_out,
    n >= 2^32 - 1 and a workspace one byte short are NSX_EINVAL before anything else; a well-formed call on a host with
    no GPU is then NSX_ENODEV, n == 0 (where d_base, d_valid and d_order may be NULL) included."""
    flow = "_flow_" in name
    bad = [dict(base=None), dict(offsets=None), dict(valid=None), dict(work=None), dict(out="null"),
           dict(n=0xFFFFFFFF, work_bytes=1 << 62), dict(n=1 << 32, work_bytes=1 << 62),
           dict(work_bytes=_need(name, 100) - 1), dict(work_bytes=0), dict(n=0, work_bytes=_need(name, 0) - 1),
           dict(n=0, offsets=None), dict(n=0, work=None), dict(n=0, out="null")]
    if flow:
        bad += [dict(order=None), dict(work_bytes=nsx.ugro_work_bytes(100))]
    for kw in bad:
        assert _call(name, tuned=tuned, **kw) == E, kw
    for k, _, _ in nsx.UGRO_FIELDS:
        assert _call(name, tuned=tuned, out=_out(null=(k,))) == E, k
        assert _call(name, tuned=tuned, n=0, out=_out(null=(k,))) == E, k
    if nsx.device_count() == 0:
        assert _call(name, tuned=tuned) == D
        assert _call(name, tuned=tuned, n=0, base=None, valid=None, order=None) == D
        assert _call(name, tuned=tuned, n=0xFFFFFFFE, work_bytes=1 << 62) == D


def test_ugro_work_bytes():
    """Both monotone in n; the plain value holds the per-frame scratch (a destination offset, a meta dword and a last
    frame per frame, block sums for the smallest scan block); the flow value is at least the plain value plus the four
    key / index buffers and the digit table of the smallest tile; both refuse n >= 2^32 - 1 and a NULL out."""
    ns = (0, 1, 15, 16, 17, 255, 256, 257, 4096, 4097, 1 << 20, 0xFFFFFFFE)
    w = [nsx.ugro_work_bytes(n) for n in ns]
    wf = [nsx.ugro_flow_work_bytes(n) for n in ns]
    assert all(b > a for a, b in zip(w, w[1:])) and all(b > a for a, b in zip(wf, wf[1:]))
    for n, a, b in zip(ns, w, wf):
        assert a >= 16 * n + 16 * ((n + 15) // 16) + 8, n
        assert b >= a + 16 * n + 4 * 256 * ((n + 255) // 256), n
        assert b <= a + 20 * n + 2048, n
    L = nsx.lib()
    c = ctypes.c_uint64(0)
    for fn in (L.nsx_ugro_work_bytes, L.nsx_ugro_flow_work_bytes):
        assert fn(0xFFFFFFFF, ctypes.byref(c)) == E and fn(1 << 40, ctypes.byref(c)) == E and fn(5, None) == E
        assert fn(0xFFFFFFFE, ctypes.byref(c)) == nsx.NSX_OK
    for f in (nsx.ugro_work_bytes, nsx.ugro_flow_work_bytes):
        with pytest.raises(nsx.NsxError) as e:
            f(0xFFFFFFFF)
        assert e.value.code == E


@pytest.mark.parametrize("flow", [False, True], ids=["adjacent", "flow"])
def test_ugro_binding_checks_extents_before_the_c_call(flow):
    """Every given tensor's extent and dtype is checked before the C call (CPU tensors here: a well-formed call is then
    refused as not on a device)."""
    import torch
    n = 70
    offs = torch.arange(n + 1, dtype=torch.int64) * 60
    buf = torch.zeros(60 * n, dtype=torch.uint8)
    valid = torch.zeros(2, dtype=torch.int64)
    need = nsx.ugro_flow_work_bytes(n) if flow else nsx.ugro_work_bytes(n)
    for ipver in (4, 6):
        fn = getattr(nsx, f"ugro_flow_ipv{ipver}_dev" if flow else f"ugro_ipv{ipver}_dev")
        alen = 4 if ipver == 4 else 16
        cases = [(dict(valid=valid[:1]), " valid"), (dict(valid=None), "`valid` is required"),
                 (dict(valid=torch.zeros(4, dtype=torch.int32)), "8-byte elements"),
                 (dict(offsets=offs.to(torch.int32)), "8-byte elements"),
                 (dict(buf=buf.view(torch.int16)), "1-byte elements"),
                 (dict(work=torch.zeros(need - 1, dtype=torch.uint8)), " work"),
                 (dict(out={"bogus": buf}), "unknown output"),
                 (dict(out={"seq_num": buf}), "unknown output"),
                 (dict(out={"src": torch.zeros(alen * n - 1, dtype=torch.uint8)}), " src"),
                 (dict(out={"gso": torch.zeros(n, dtype=torch.int16)}), "4-byte elements"),
                 (dict(out={"gso": torch.zeros(n - 1, dtype=torch.int32)}), " gso"),
                 (dict(out={"data": torch.zeros(60 * n - 1, dtype=torch.uint8)}), " data:"),
                 (dict(out={"data_off": torch.zeros(n, dtype=torch.int64)}), " data_off"),
                 (dict(out={"n_super": torch.zeros(1, dtype=torch.int32)}), "8-byte elements"),
                 (dict(out={"frame_seg": torch.zeros(n - 1, dtype=torch.int32)}), " frame_seg:")]
        if flow:
            cases += [(dict(order=torch.zeros(n - 1, dtype=torch.int32)), " order"),
                      (dict(order=torch.zeros(n, dtype=torch.int64)), "4-byte elements"),
                      (dict(work=torch.zeros(nsx.ugro_work_bytes(n), dtype=torch.uint8)), " work")]
        cases.append((dict(), "device"))
        for kw, msg in cases:
            args = dict(buf=buf, offsets=offs, valid=valid)
            args.update(kw)
            with pytest.raises(ValueError) as e:
                fn(**args)
            assert msg in str(e.value), (msg, str(e.value))
            assert fn.__name__ in str(e.value) or msg == "device"


# ---------------------------------------------------------------- the model, held to what exists
def _cut_lengths(gso):
    return sorted({0, 1, gso - 1, gso, gso + 1, 3 * gso - 1, 3 * gso, 3 * gso + 1})


def _assert_same_frames(buf, offs, buf2, offs2, n):
    assert offs2.size - 1 == n
    for p in range(n):
        assert buf2[int(offs2[p]):int(offs2[p + 1])].tobytes() == buf[int(offs[p]):int(offs[p + 1])].tobytes(), p


@pytest.mark.parametrize("gso", [1, 7, 512, 1472])
@pytest.mark.parametrize("ipver", [4, 6])
def test_model_inverts_segmentation_offload(ipver, gso):
    """expand → frames → the receive verify → ugro gives a super-datagram batch back — fields, gso, data, frame map —
    for every cut length of one gso, and the expansion of the model's output reproduces the input frames. Every super-
    datagram is a flow of its own (random addresses and ports), so nothing merges across them."""
    rng = np.random.default_rng([0x06B0, ipver, gso])
    lens = np.array(_cut_lengths(gso) * 2)
    rng.shuffle(lens)
    b = _udp.Batch(rng, ipver, lens, gso, lead=int(rng.integers(4)))
    buf, offs = UG.frames_of(b, lead=int(rng.integers(4)))
    valid, _, _ = _udp.rx_expected(ipver, buf, offs)
    assert valid.all()
    out = UG.ugro(buf, offs, valid, ipver)
    s = b.sup
    assert out["n_super"] == b.n
    # a super-datagram of at most one datagram comes back with gso = max(len, 1): the expansion is the same frame
    want_gso = np.where(s.plen <= b.gso, np.maximum(s.plen, 1), b.gso).astype(np.uint32)
    assert np.array_equal(out["gso"], want_gso)
    assert np.array_equal(out["data"], s.data[int(s.data_off[0]):int(s.data_off[-1])])
    assert np.array_equal(out["data_off"], s.data_off - s.data_off[0])
    assert np.array_equal(out["first_frame"], b.first[:-1]) and np.array_equal(out["frame_cnt"], np.diff(b.first))
    assert np.array_equal(out["frame_seg"], b.seg)
    for k in ("src", "dst", "ttl"):
        assert np.array_equal(out[k], s.ip[k]), k
    for k in ("src_port", "dst_port"):
        assert np.array_equal(out[k], s.ports[k]), k
    if ipver == 4:
        assert np.array_equal(out["ident"], s.ip["ident"]) and not out["flow"].any() and not out["tclass"].any()
    else:
        assert not out["ident"].any() and np.array_equal(out["tclass"], s.ip["tclass"])
        assert np.array_equal(out["flow"], s.ip["flow"] & np.uint32(0xFFFFF))
    b2 = UG.as_batch(out, ipver)
    buf2, offs2 = UG.frames_of(b2)
    _assert_same_frames(buf, offs, buf2, offs2, b.nf)


def _hand(ipver, frames, valid=None):
    buf, offs = UG.pack(frames, lead=1)
    valid = np.ones(len(frames), bool) if valid is None else np.asarray(valid, bool)
    return UG.ugro(buf, offs, valid, ipver), buf, offs


@pytest.mark.parametrize("ipver", [4, 6])
def test_model_hand_cases(ipver):
    rng = np.random.default_rng(0x06B1 + ipver)
    h = UG.IPH[ipver]
    # strictly decreasing payloads lose merges to the three-frame window
    out, _, _ = _hand(ipver, UG.flow_frames(rng, ipver, [1000, 800, 600, 400, 200]))
    assert out["frame_cnt"].tolist() == [2, 1, 1, 1] and out["gso"].tolist() == [1000, 600, 400, 200]
    assert out["frame_seg"].tolist() == [0, 0, 1, 2, 3] and out["data_off"].tolist() == [0, 1800, 2400, 2800, 3000]
    # a run and its short tail; the frame behind the tail starts anew
    out, _, _ = _hand(ipver, UG.flow_frames(rng, ipver, [700, 700, 700, 300, 700, 700]))
    assert out["frame_cnt"].tolist() == [4, 2] and out["gso"].tolist() == [700, 700]
    # a zero-payload datagram is a member, never joins and is never joined: gso 1, no data
    out, _, _ = _hand(ipver, UG.flow_frames(rng, ipver, [10, 0, 0, 10]))
    assert out["frame_cnt"].tolist() == [1, 1, 1, 1] and out["gso"].tolist() == [10, 1, 1, 10]
    assert out["data_off"].tolist() == [0, 10, 10, 10, 20]
    fr = UG.flow_frames(rng, ipver, [64] * 6, ident0=0xFFFD)  # the ident wraps at 0xFFFF inside the run
    out, _, _ = _hand(ipver, fr)
    assert out["frame_cnt"].tolist() == [6]
    assert out["ident"].tolist() == ([0xFFFD] if ipver == 4 else [0])

    def edit(k, fn, fix=True):
        g = [bytearray(f) for f in fr]
        fn(g[k])
        return [UG.refix(f, ipver) if fix else bytes(f) for f in g]

    def zero_field(f):
        f[h + 6:h + 8] = b"\0\0"
    # a zero checksum field: valid to the IPv4 verify, never a member
    g = edit(2, zero_field, fix=False)
    valid, _, _ = _udp.rx_expected(ipver, *UG.pack(g, lead=1))
    assert valid.tolist() == [True, True, ipver == 4, True, True, True]
    out, _, _ = _hand(ipver, g)  # with every bit set, as a wrong mask would have it
    assert out["frame_cnt"].tolist() == [2, 3] and out["frame_seg"].tolist() == [0, 0, UG.NONE, 1, 1, 1]
    # a padded datagram (U < P) is valid to the verify and no member
    pad = [bytes(_udp.corrupt(rng, np.frombuffer(f, np.uint8), ipver, "padding")) if k == 3 else f
           for k, f in enumerate(fr)]
    valid, _, _ = _udp.rx_expected(ipver, *UG.pack(pad, lead=1))
    assert valid.all()
    out, _, _ = _hand(ipver, pad)
    assert out["frame_cnt"].tolist() == [3, 2] and out["frame_seg"][3] == UG.NONE

    def ttl(f):
        f[8 if ipver == 4 else 7] ^= 1

    def port(f):
        f[h + 3] ^= 1
    for fn in (ttl, port):
        out, _, _ = _hand(ipver, edit(3, fn))
        assert out["frame_cnt"].tolist() == [3, 1, 2], fn.__name__  # one frame differs: it is alone
    if ipver == 4:
        def gap(f):
            f[4:6] = ((int.from_bytes(f[4:6], "big") + 1) & 0xFFFF).to_bytes(2, "big")
        out, _, _ = _hand(ipver, edit(3, gap))  # frame 3 has frame 4's ident: 2 → 3 breaks, and so does 3 → 4
        assert out["frame_cnt"].tolist() == [3, 1, 2]

        def tos(f):
            f[1] = 0x10
        out, _, _ = _hand(ipver, edit(3, tos))
        assert out["frame_cnt"].tolist() == [3, 1, 2] and out["tclass"].tolist() == [0, 0x10, 0]
    else:
        def label(f):
            f[3] ^= 1
        out, _, _ = _hand(ipver, edit(3, label))
        assert out["frame_cnt"].tolist() == [3, 1, 2]
    # a clear valid bit inside a run: the frame is not looked at and breaks the run
    valid = np.ones(6, bool)
    valid[2] = False
    out, _, _ = _hand(ipver, fr, valid)
    assert out["frame_cnt"].tolist() == [2, 3] and out["frame_seg"].tolist() == [0, 0, UG.NONE, 1, 1, 1]
    assert out["first_frame"].tolist() == [0, 3]


@pytest.mark.parametrize("ipver", [4, 6])
def test_model_key_definition(ipver):
    """The key by hand; a non-member's is 0xFFFFFFFF; ports crafted as tests/_gro_flow.ports_for_key does hit the key
    asked for."""
    rng = np.random.default_rng(0x06B2 + ipver)
    f = UG.flow_frames(rng, ipver, [100])[0]
    ihl = UG.IPH[ipver]
    hsh = 0x811C9DC5
    raw = (f[12:20] if ipver == 4 else f[8:40]) + f[ihl:ihl + 4]
    for k in range(0, len(raw), 4):
        hsh = ((hsh ^ int.from_bytes(raw[k:k + 4], "little")) * 0x01000193) % (1 << 32)
    assert UG.key(f, ipver) == hsh != UG.NO_FLOW
    bad = bytearray(f)
    bad[ihl + 6:ihl + 8] = b"\0\0"
    assert UG.key(bytes(bad), ipver) == UG.NO_FLOW and UG.key(f[:-1], ipver) == UG.NO_FLOW
    for k in (0, 1, 0xFFFFFFFF, 0x12345678):
        g = UG.with_ports(f, ipver, FL.ports_for_key(FL.state(f, ipver), k))
        assert UG.key(g, ipver) == k and UG.parse(g, ipver) is not None
        assert _udp.rx_expected(ipver, *UG.pack([g]))[0].all()


@pytest.mark.parametrize("ipver", [4, 6])
def test_model_flow_round_robin_coalesces_fully(ipver):
    """5 flows x 4 datagrams (700, 700, 700, 300) delivered round-robin: nothing merges by adjacency, every flow
    merges whole by key; one flow is alone: `order` is the identity and every array the adjacent model's; expanding
    the output reproduces frame order[p] at position p."""
    rng = np.random.default_rng(0x06B3 + ipver)
    flows = [UG.flow_frames(rng, ipver, [700, 700, 700, 300]) for _ in range(5)]
    frames, who = FL.round_robin(flows)
    buf, offs = UG.pack(frames, lead=3)
    valid = np.ones(20, bool)
    assert UG.ugro(buf, offs, valid, ipver)["n_super"] == 20
    out = UG.ugro_flow(buf, offs, valid, ipver)
    od = out["order"]
    assert out["n_super"] == 5 and out["frame_cnt"].tolist() == [4] * 5 and sorted(od.tolist()) == list(range(20))
    for s in range(5):
        pos = od[4 * s:4 * s + 4]
        assert len({who[p] for p in pos}) == 1 and list(pos) == sorted(pos)
        assert (out["frame_seg"][pos] == s).all() and out["first_frame"][s] == 4 * s
    b2 = UG.as_batch(out, ipver)
    buf2, offs2 = UG.frames_of(b2)
    for p in range(20):
        f = int(od[p])
        assert buf2[int(offs2[p]):int(offs2[p + 1])].tobytes() == buf[int(offs[f]):int(offs[f + 1])].tobytes(), p
    one, o1 = UG.pack(flows[0], lead=1)
    a, b = UG.ugro(one, o1, np.ones(4, bool), ipver), UG.ugro_flow(one, o1, np.ones(4, bool), ipver)
    assert b["order"].tolist() == [0, 1, 2, 3]
    for k, v in a.items():
        assert np.array_equal(b[k], v), k


@pytest.mark.parametrize("ipver", [4, 6])
def test_model_colliding_keys_never_merge_wrongly(ipver):
    """Two flows given one key interleave in the order as they arrived: same() keeps them apart, the collision costs
    every merge; a member whose key is 0xFFFFFFFF sorts among the non-members."""
    rng = np.random.default_rng(0x06B4 + ipver)
    a = UG.flow_frames(rng, ipver, [200] * 4)
    b = UG.flow_frames(rng, ipver, [200] * 4)
    ka = UG.key(a[0], ipver)
    b = [UG.with_ports(f, ipver, FL.ports_for_key(FL.state(f, ipver), ka)) for f in b]
    assert {UG.key(f, ipver) for f in a + b} == {ka}
    frames, _ = FL.round_robin([a, b])
    buf, offs = UG.pack(frames)
    out = UG.ugro_flow(buf, offs, np.ones(8, bool), ipver)
    assert out["order"].tolist() == list(range(8)) and out["n_super"] == 8
    c = [UG.with_ports(f, ipver, FL.ports_for_key(FL.state(f, ipver), 0xFFFFFFFF)) for f in a]
    valid = np.array([True, False] * 4)
    frames, _ = FL.round_robin([c, b])
    buf, offs = UG.pack(frames)
    out = UG.ugro_flow(buf, offs, valid, ipver)
    assert out["order"].tolist() == list(range(8))  # every key is 0xFFFFFFFF
    assert out["n_super"] == 4 and out["frame_seg"].tolist() == [0, UG.NONE, 1, UG.NONE, 2, UG.NONE, 3, UG.NONE]
