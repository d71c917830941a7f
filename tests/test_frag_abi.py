"""IPv4 fragmentation and reassembly's boundary (nsx_frag_*, nsx_reasm_*), on any host: the symbols, every NSX_EINVAL
before NSX_ENODEV, the host helpers against the numpy restatement tests/_frag.py, the workspace size, the binding's extent
checks, and the model held to its own round trip and to the receive verifies that already exist. The GPU tests
(tests/test_gpu_frag.py, tests/test_gpu_reasm.py, tests/test_gpu_frag_fuzz.py) compare the kernels against tests/_frag.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nsx
import _far
import _frag as F
import _udp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CALLS = ("nsx_frag_count_host", "nsx_frag_layout_host")
DEV_CALLS = ("nsx_frag_ipv4_dev", "nsx_reasm_ipv4_dev")
fake = ctypes.c_void_p(0x1000)
E, D, OK = nsx.NSX_EINVAL, nsx.NSX_ENODEV, nsx.NSX_OK


# ---------------------------------------------------------------- symbols
def test_frag_symbols_are_declared_and_exported(tmp_path):
    """nsx_csum.h declares exactly the three nsx_frag_* and the two nsx_reasm_* calls and nsx_frag_tune.h exactly the
    two _tuned twins; that header brings nsx_tune.h in and no other tune header names the calls; the library exports
    all seven; the closed sets of the older families are what they were; the ABI version stays 2; the header states
    the contract; a plain C caller compiles with -Wall -Werror and gets the documented codes."""
    inc = os.path.join(ROOT, "include")
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)  # noqa: E731
    decl = r"^int\s+(nsx_(?:frag|reasm)_[a-z_0-9]+)\("
    text = open(os.path.join(inc, "nsx_csum.h")).read()
    mine = set(HOST_CALLS) | set(DEV_CALLS) | {"nsx_reasm_work_bytes"}
    assert set(re.findall(decl, strip(text), flags=re.M)) == mine
    tune = open(os.path.join(inc, "nsx_frag_tune.h")).read()
    assert set(re.findall(decl, strip(tune), flags=re.M)) == {c + "_tuned" for c in DEV_CALLS}
    assert '#include "nsx_tune.h"' in tune
    for h in ("nsx_tune.h", "nsx_tx_tune.h", "nsx_gro_tune.h", "nsx_udp_tune.h", "nsx_ugro_tune.h"):
        t = open(os.path.join(inc, h)).read()
        assert "nsx_frag_" not in t and "nsx_reasm_" not in t, h
    assert len(re.findall(r"^int\s+nsx_\w+\(", strip(open(os.path.join(inc, "nsx_tune.h")).read()), flags=re.M)) == 16
    out = subprocess.run(["nm", "-D", "--defined-only", nsx.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (nsx_\w+)", out))
    assert {s for s in exported if s.startswith(("nsx_frag_", "nsx_reasm_"))} == mine | {c + "_tuned" for c in DEV_CALLS}
    for prefix, cnt in (("nsx_udp_", 14), ("nsx_gro_", 10), ("nsx_ugro_", 10), ("nsx_nat_", 4)):
        assert len([s for s in exported if s.startswith(prefix)]) == cnt, prefix
    assert nsx.abi_version() == 2 and "NSX_ABI_VERSION 2 " in text
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for word in ("IPv4 fragmentation and reassembly (RFC 791", "IPv4 only: IPv6 fragments in an extension header",
                 "per_i = (mtu_i - 20) & ~7", "is dense, out_off[0] = 0, no padding", "a frame of 2^30 bytes or more",
                 "which keeps the frame's own MF", "RFC 1624 eqn. 3 with the fold defined for nsx_nat_* above",
                 "every byte of the frame's slots is written as zero", "the caller owes an ICMP",
                 "There is no validity mask", "the raw sum over its 20 header bytes is 0xFFFF",
                 "o*8 + pay <= 65515", "b4 | b5<<8 | b9<<16", "numpy.lexsort((arrival, off, key))",
                 "an overlap, a gap or a duplicate breaks the run", "A member with no datagram is a leftover",
                 "There are no timers and no cross-batch state", "RFC 4963",
                 "rebuilds every cut frame byte for byte, in any order of the fragments",
                 "frames may lie past 2^32 in d_base"):
        assert word in flat, word
    flat_tune = re.sub(r"\s*\n \*\s*", " ", tune)
    assert "keys per tile of the radix sort in units of 256" in flat_tune and "clamped to 16..65536" in flat_tune
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include "nsx_csum.h"
#include "nsx_frag_tune.h"
int main(void) {
    nsx_reasm_out o = {0};
    nsx_tune t = {0};
    uint64_t need = 0, offs[3] = {0, 3000, 3100}, first[3], out_off[5];
    uint32_t mtu[2] = {1500, 1500}, src[4], order[1];
    uint8_t st[2];
    if (nsx_frag_count_host(offs, mtu, 2, first) != NSX_OK || first[2] != 4) return 1;
    if (nsx_frag_layout_host(offs, mtu, first, 2, src, out_off) != NSX_OK || out_off[4] != 3140 || src[3] != 1) return 2;
    if (nsx_reasm_work_bytes(1000, &need) != NSX_OK || need < 44 * 1000) return 3;
    if (nsx_reasm_work_bytes(0xFFFFFFFFull, &need) != NSX_EINVAL || nsx_reasm_work_bytes(1, 0) != NSX_EINVAL) return 4;
    if (nsx_frag_ipv4_dev(offs, offs, mtu, 2, first, src, 1, st, out_off, st, 0) != NSX_EINVAL) return 5;
    if (nsx_frag_ipv4_dev_tuned(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, &t) != NSX_OK) return 6;
    if (nsx_reasm_ipv4_dev(offs, offs, 0, order, &o, offs, 1 << 20, 0) != NSX_EINVAL) return 7;
    if (nsx_reasm_ipv4_dev_tuned(offs, offs, 0, order, 0, offs, 1 << 20, 0, &t) != NSX_EINVAL) return 8;
    return NSX_FRAG_PASS + NSX_FRAG_CUT + NSX_FRAG_DF + NSX_FRAG_BAD - 6;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(nsx.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I", inc, "-L", libdir, "-lnsx_csum",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- validation
def _frag_call(tuned=False, **kw):
    a = dict(base=fake, offsets=fake, mtu=fake, n=100, first=fake, src=fake, n_frags=150, out=fake, out_off=fake,
             status=fake)
    a.update(kw)
    args = [a["base"], a["offsets"], a["mtu"], a["n"], a["first"], a["src"], a["n_frags"], a["out"], a["out_off"],
            a["status"], None]
    if tuned:
        return nsx.lib().nsx_frag_ipv4_dev_tuned(*args, ctypes.byref(nsx.Tune(blocks_per_cu=1)))
    return nsx.lib().nsx_frag_ipv4_dev(*args)


@pytest.mark.parametrize("tuned", [False, True], ids=["plain", "tuned"])
def test_frag_device_call_validates_before_any_device_work(tuned):
    """Every NULL array with n > 0, n >= 2^32, fewer slots than frames and slots without frames are NSX_EINVAL before
    anything else; n_frags == 0 is NSX_OK without a launch, with or without a GPU; a well-formed call on a host with no
    GPU is then NSX_ENODEV."""
    bad = [dict(base=None), dict(offsets=None), dict(mtu=None), dict(first=None), dict(src=None), dict(out=None),
           dict(out_off=None), dict(status=None), dict(n=1 << 32, n_frags=1 << 33), dict(n_frags=99),
           dict(n=0, n_frags=1), dict(n=5, n_frags=0)]
    for kw in bad:
        assert _frag_call(tuned, **kw) == E, kw
    assert _frag_call(tuned, n=0, n_frags=0) == OK
    assert _frag_call(tuned, n=0, n_frags=0, base=None, offsets=None, mtu=None, first=None, src=None, out=None,
                      out_off=None, status=None) == OK
    if nsx.device_count() == 0:
        assert _frag_call(tuned) == D
        assert _frag_call(tuned, n=0xFFFFFFFF, n_frags=1 << 32) == D


def _rout(null=()):
    return nsx.ReasmOut(*[None if k in null else 0x1000 for k, _, _ in nsx.REASM_FIELDS])


def _reasm_call(n=100, tuned=False, out=None, **kw):
    a = dict(base=fake, offsets=fake, order=fake, work=fake, work_bytes=nsx.reasm_work_bytes(min(n, 1 << 20)))
    a.update(kw)
    o = _rout() if out is None else out
    args = [a["base"], a["offsets"], n, a["order"], None if o == "null" else ctypes.byref(o), a["work"],
            a["work_bytes"], None]
    if tuned:
        return nsx.lib().nsx_reasm_ipv4_dev_tuned(*args, ctypes.byref(nsx.Tune(rows=1, run_segs=16, blocks_per_cu=1)))
    return nsx.lib().nsx_reasm_ipv4_dev(*args)


@pytest.mark.parametrize("tuned", [False, True], ids=["plain", "tuned"])
def test_reasm_device_call_validates_before_any_device_work(tuned):
    """NULL pointers (d_base and d_order with n > 0), every NULL member of nsx_reasm_out, n >= 2^32 - 1 and a workspace
    one byte short are NSX_EINVAL before anything else; a well-formed call on a host with no GPU is then NSX_ENODEV,
    n == 0 (where d_base and d_order may be NULL) included."""
    need = nsx.reasm_work_bytes
    bad = [dict(base=None), dict(offsets=None), dict(order=None), dict(work=None), dict(out="null"),
           dict(n=0xFFFFFFFF, work_bytes=1 << 62), dict(n=1 << 32, work_bytes=1 << 62),
           dict(work_bytes=need(100) - 1), dict(work_bytes=0), dict(n=0, work_bytes=need(0) - 1),
           dict(n=0, offsets=None), dict(n=0, work=None), dict(n=0, out="null")]
    for kw in bad:
        assert _reasm_call(tuned=tuned, **kw) == E, kw
    for k, _, _ in nsx.REASM_FIELDS:
        assert _reasm_call(tuned=tuned, out=_rout(null=(k,))) == E, k
        assert _reasm_call(tuned=tuned, n=0, out=_rout(null=(k,))) == E, k
    if nsx.device_count() == 0:
        assert _reasm_call(tuned=tuned) == D
        assert _reasm_call(tuned=tuned, n=0, base=None, order=None) == D
        assert _reasm_call(tuned=tuned, n=0xFFFFFFFE, work_bytes=1 << 62) == D


def test_reasm_work_bytes_is_monotone():
    """Monotone in n; it holds the per-frame scratch (a meta dword, a run, three per-run dwords and an offset, the
    key), block sums for the smallest scan block, and the sort's four buffers with the digit table of the smallest tile;
    it refuses n >= 2^32 - 1 and a NULL out."""
    ns = (0, 1, 15, 16, 17, 255, 256, 257, 4096, 4097, 1 << 20, 0xFFFFFFFE)
    w = [nsx.reasm_work_bytes(n) for n in ns]
    assert all(b > a for a, b in zip(w, w[1:]))
    for n, a in zip(ns, w):
        assert a >= 28 * n + 16 * ((n + 15) // 16) + 16 * n + 4 * 256 * ((n + 255) // 256), n
        assert a <= 50 * n + 4096, n
    c = ctypes.c_uint64(0)
    fn = nsx.lib().nsx_reasm_work_bytes
    assert fn(0xFFFFFFFF, ctypes.byref(c)) == E and fn(1 << 40, ctypes.byref(c)) == E and fn(5, None) == E
    assert fn(0xFFFFFFFE, ctypes.byref(c)) == OK
    with pytest.raises(nsx.NsxError) as e:
        nsx.reasm_work_bytes(0xFFFFFFFF)
    assert e.value.code == E


def test_binding_checks_extents_before_the_c_call():
    """Every given tensor's extent and dtype is checked before the C call (CPU tensors here: a well-formed call is then
    refused as not on a device)."""
    import torch
    n = 70
    offs = torch.arange(n + 1, dtype=torch.int64) * 60
    buf = torch.zeros(60 * n, dtype=torch.uint8)
    need = nsx.reasm_work_bytes(n)
    cases = [(dict(offsets=offs.to(torch.int32)), "8-byte elements"), (dict(buf=buf.view(torch.int16)), "1-byte elements"),
             (dict(work=torch.zeros(need - 1, dtype=torch.uint8)), " work"),
             (dict(out={"bogus": buf}), "unknown output"), (dict(out={"out": buf[:-1]}), " out:"),
             (dict(out={"out_off": torch.zeros(n, dtype=torch.int64)}), " out_off"),
             (dict(out={"frag_cnt": torch.zeros(n, dtype=torch.int16)}), "4-byte elements"),
             (dict(out={"frame_seg": torch.zeros(n - 1, dtype=torch.int32)}), " frame_seg:"),
             (dict(out={"is_frag": torch.zeros(1, dtype=torch.int64)}), " is_frag"),
             (dict(out={"n_out": torch.zeros(1, dtype=torch.int32)}), "8-byte elements"),
             (dict(order=torch.zeros(n - 1, dtype=torch.int32)), " order"),
             (dict(order=torch.zeros(n, dtype=torch.int64)), "4-byte elements"), (dict(), "device")]
    for kw, msg in cases:
        args = dict(buf=buf, offsets=offs)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            nsx.reasm_ipv4_dev(**args)
        assert msg in str(e.value), (msg, str(e.value))
    mtu = torch.full((n,), 28, dtype=torch.int32)
    first = torch.arange(n + 1, dtype=torch.int64) * 5
    src = torch.zeros(5 * n, dtype=torch.int32)
    out_off = torch.zeros(5 * n + 1, dtype=torch.int64)
    good = dict(buf=buf, offsets=offs, mtu=mtu, frag_first=first, frag_src=src, out=buf, out_off=out_off)
    cases = [(dict(mtu=mtu[:-1]), " mtu"), (dict(mtu=mtu.to(torch.int64)), "4-byte elements"),
             (dict(frag_first=first[:-1]), " frag_first"), (dict(frag_src=src[:-1]), " frag_src"),
             (dict(frag_src=src.to(torch.int64)), "4-byte elements"), (dict(out_off=out_off[:n]), "slots for"),
             (dict(out=buf.view(torch.int16)), "1-byte elements"),
             (dict(status=torch.zeros(n - 1, dtype=torch.uint8)), " status"),
             (dict(n_frags=5 * n + 1), " frag_src"), (dict(), "device")]
    for kw, msg in cases:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            nsx.frag_ipv4_dev(**args)
        assert msg in str(e.value), (msg, str(e.value))


# ---------------------------------------------------------------- the host helpers against the model
HAND = [  # (frame lengths, mtus)
    ([1500], [1500]),            # len == mtu: one slot, the frame
    ([1501], [1500]),            # len == mtu + 1: 1480 + 1
    ([29, 28, 100, 21], [28, 28, 28, 28]),   # mtu 28: pieces of 8 bytes
    ([20 + 3 * 1480], [1500]),   # a remainder of exactly per
    ([20 + 3 * 1480 + 1], [1500]),
    ([0, 0, 3000, 0], [576, 28, 576, 1500]),  # empty frames take a slot of no bytes
    ([65535, 9000, 577, 576], [68, 4100, 576, 576]),
    ([], []),
]


def _offsets(lens, lead=0):
    o = np.zeros(len(lens) + 1, np.uint64)
    o[1:] = np.cumsum(np.asarray(lens, np.uint64)) if len(lens) else 0
    return o + np.uint64(lead)


def _same_map(lens, mtus, lead=0):
    offs, mtu = _offsets(lens, lead), np.asarray(mtus, np.uint32)
    first = nsx.frag_count_host(offs, mtu)
    assert np.array_equal(first, F.count(offs, mtu))
    src, off = nsx.frag_layout_host(offs, mtu, first)
    wsrc, woff = F.layout(offs, mtu, first)
    assert np.array_equal(src, wsrc) and np.array_equal(off, woff)
    return first, src, off


def test_host_helpers_hand_cases():
    for lens, mtus in HAND:
        _same_map(lens, mtus, lead=7)
    first, src, off = _same_map([1501], [1500])
    assert first.tolist() == [0, 2] and np.diff(off).tolist() == [1500, 21]
    first, src, off = _same_map([20 + 3 * 1480], [1500])
    assert first.tolist() == [0, 3] and np.diff(off).tolist() == [1500] * 3
    first, src, off = _same_map([29], [28])
    assert first.tolist() == [0, 2] and np.diff(off).tolist() == [28, 21]
    first, src, off = _same_map([0, 0, 3000, 0], [576, 28, 576, 1500])
    assert first.tolist() == [0, 1, 2, 8, 9] and src.tolist() == [0, 1, 2, 2, 2, 2, 2, 2, 3]


def test_host_helpers_on_200_seeded_batches():
    for seed in range(200):
        rng = np.random.default_rng([0xF4A6, seed])
        n = int(rng.integers(0, 40))
        mtus = rng.choice([28, 36, 68, 576, 1500, 4100, 9000, 65535], n)
        lens = [int(rng.choice([0, 1, 20, 21, m - 1, m, m + 1, 20 + 3 * ((m - 20) & ~7), int(rng.integers(0, 70000))]))
                for m in mtus]
        _same_map(lens, mtus, lead=int(rng.integers(0, 1 << 34)))


def test_host_helpers_refuse_and_write_nothing():
    L = nsx.lib()
    offs, mtu = _offsets([3000, 100]), np.array([1500, 1500], np.uint32)
    first = np.full(3, 77, np.uint64)
    src, off = np.full(4, 77, np.uint32), np.full(5, 77, np.uint64)
    p = nsx._np_ptr
    good_first = nsx.frag_count_host(offs, mtu)
    bad = [(None, p(mtu), 2), (p(offs), None, 2), (p(offs), p(mtu), 1 << 32), (p(_offsets([5, 1])[::-1].copy()), p(mtu), 2),
           (p(offs), p(np.array([1500, 27], np.uint32)), 2), (p(np.array([0, 1 << 30], np.uint64)), p(mtu), 1)]
    for a, b, n in bad:
        assert L.nsx_frag_count_host(a, b, n, p(first)) == E
        assert L.nsx_frag_layout_host(a, b, p(good_first), n, p(src), p(off)) == E
    assert L.nsx_frag_count_host(p(offs), p(mtu), 2, None) == E
    wrong = good_first.copy()
    wrong[1] += 1
    for f, s, o in ((p(wrong), p(src), p(off)), (None, p(src), p(off)), (p(good_first), None, p(off)),
                    (p(good_first), p(src), None)):
        assert L.nsx_frag_layout_host(p(offs), p(mtu), f, 2, s, o) == E
    assert (first == 77).all() and (src == 77).all() and (off == 77).all()
    assert F.count(_offsets([5, 1])[::-1], mtu) is None and F.count(offs, [1500, 27]) is None
    assert F.layout(offs, mtu, wrong) is None
    with pytest.raises(nsx.NsxError):
        nsx.frag_count_host(offs, np.array([1500, 27], np.uint32))


# ---------------------------------------------------------------- the model, held to what exists
def _round_trip(frames, mtu, rng, lead=0):
    slots, status = F.frag_frames(frames, mtu)
    perm = rng.permutation(len(slots))
    buf, offs = F.pack([slots[i] for i in perm], lead=lead)
    res = F.reasm(buf, offs)
    return slots, status, perm, res


@pytest.mark.parametrize("mtu", [28, 68, 576, 1500])
def test_model_round_trip_is_the_identity(mtu):
    """frag → shuffle → reasm gives every cut frame back byte for byte; the frames that fit pass through and are no
    members; every fragment's header checksum is valid and equals a full recomputation."""
    rng = np.random.default_rng([0xF4A7, mtu])
    per = F.per_of(mtu)
    pays = [1, 7, 8, 9, mtu - 28, mtu - 27, per, per + 1, 3 * per, 3 * per + 8, 3 * per - 8 - 1, 2000]
    frames = F.udp_frames(rng, pays) + F.tcp_frames(rng, [0, 1, per, 1460, 3000])
    slots, status, perm, res = _round_trip(frames, mtu, rng, lead=3)
    cut = [f for f, s in zip(frames, status) if s == F.CUT]
    assert len(cut) >= 8 and all(s in (F.PASS, F.CUT) for s in status)
    for s in slots:
        assert _udp.fix4(np.frombuffer(s, np.uint8)).tobytes() == s
    assert sorted(F.datagrams(res)) == sorted(cut)
    n_frag = sum(len(s) > 20 and bool(F.member(s)) for s in slots)
    assert (res["frame_seg"] != F.NONE).sum() == n_frag == int(res["frag_cnt"].sum())
    assert sum(bin(int(w)).count("1") for w in res["is_frag"]) == n_frag


def test_model_reassembled_datagrams_pass_the_receive_verifies():
    """The model's reassembled UDP datagrams pass tests/_udp.rx_expected and its TCP datagrams the receive pass's
    oracle; a fragment alone passes neither."""
    rng = np.random.default_rng(0xF4A8)
    u, t = F.udp_frames(rng, [1473, 3000, 20000, 65507]), F.tcp_frames(rng, [1461, 5000, 30000])
    for frames, verify in ((u, lambda b, o: _udp.rx_expected(4, b, o)[0]),
                           (t, lambda b, o: np.unpackbits(_far.rx_model(4, b, o)[0].view(np.uint8),
                                                          bitorder="little")[:len(frames)].astype(bool))):
        slots, status, perm, res = _round_trip(frames, 1500, rng)
        assert (status == F.CUT).all() and res["n_out"] == len(frames)
        buf, offs = F.pack(F.datagrams(res))
        assert verify(buf, offs).all()
        fb, fo = F.pack(slots[:4])
        assert not verify(fb, fo).any()
    assert len(u[-1]) == 65535  # the longest datagram IPv4 can carry came through


def test_model_hand_cases():
    rng = np.random.default_rng(0xF4A9)
    f = F.udp_frames(rng, [4000])[0]
    a, b, c = F.cut(f, 1500)
    assert [len(x) for x in (a, b, c)] == [1500, 1500, 1068]
    assert [F.member(x) for x in (a, b, c)] == [(0, 1480, True), (185, 1480, True), (370, 1048, False)]

    def run(frames):
        return F.reasm(*F.pack(frames))
    assert F.datagrams(run([c, a, b])) == [f]
    # a duplicate of the first fragment: the later copy starts the run that completes; of a middle one: two runs,
    # neither complete; of the last: the first copy closes the run
    for dup, n_out in ((a, 1), (b, 0), (c, 1)):
        r = run([a, b, c, dup])
        assert r["n_out"] == n_out and (r["n_out"] == 0 or F.datagrams(r) == [f])
    assert run([a, b, c, a])["frame_seg"].tolist() == [F.NONE, 0, 0, 0]
    r = run([a, b, c, c])  # the first copy of the last fragment closes the run, the second is a leftover
    assert r["frame_seg"].tolist() == [0, 0, 0, F.NONE] and r["is_frag"][0] == 0b1111
    # a missing first and a missing last fragment are leftovers
    for fr in ([b, c], [a, b]):
        r = run(fr)
        assert r["n_out"] == 0 and r["is_frag"][0] == 0b11 and (r["frame_seg"] == F.NONE).all()
    # a gap and an overlap
    assert run([a, c])["n_out"] == 0
    assert run([a, F.with_header(b, off=184), c])["n_out"] == 0
    # cutting a fragment again: the offsets add and the last piece keeps MF
    b1, b2, b3 = F.cut(b, 576)
    assert [F.member(x) for x in (b1, b2, b3)] == [(185, 552, True), (254, 552, True), (323, 376, True)]
    assert F.datagrams(run([b3, c, b1, a, b2])) == [f]
    # DF and a wrong checksum
    g = F.udp_frames(rng, [4000], df=True)[0]
    slots, st = F.frag_frames([g], 1500)
    assert st.tolist() == [F.DF] and not any(b"".join(slots))
    bad = bytearray(f)
    bad[10] ^= 0x55
    diff = lambda p, q: (F.be16(p, 10) - F.be16(q, 10)) % 0xFFFF  # noqa: E731
    for x, y in zip(F.cut(bytes(bad), 1500), (a, b, c)):
        assert x[:10] == y[:10] and x[12:] == y[12:] and diff(x, y) == diff(bad, f) != 0
        assert F.member(x) is None
    # RFC 4963: two datagrams with one (src, dst, ident, protocol) mix into one whose pieces abut
    g = bytearray(F.udp_frames(rng, [4000])[0])
    g[4:20] = f[4:20]
    g = F.with_header(bytes(g))
    a2, b2_, c2 = F.cut(g, 1500)
    r = run([c, b2_, a])
    assert r["n_out"] == 1 and F.datagrams(r)[0][20:] == f[20:1500] + g[1500:2980] + f[2980:]
    assert run([a, b2_, c, a2, b, c2])["n_out"] == 0  # with all six present every run breaks at a duplicate offset
