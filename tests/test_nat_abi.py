"""The NAT rewrite's boundary (nsx_nat_*), on any host: the symbols, every NSX_EINVAL before NSX_ENODEV, the binding's
extent checks, the host table builder against the restatement tests/_nat.py (collision chains, wrap-around, refusals),
and that restatement held to what already exists — frames of the transmit pass's model (tests/_tx.py), rewritten, are
the frames that model builds from the new addresses, ports and TTL. The GPU tests (tests/test_gpu_nat.py) compare the
kernel against tests/_nat.py."""
import copy
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nsx
import _gro
import _nat
import _tx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_CALLS = ("nsx_nat_ipv4_tcp_rewrite_dev", "nsx_nat_ipv6_tcp_rewrite_dev")
HOST_CALLS = ("nsx_nat_table_slots", "nsx_nat_table_build_host")
fake = ctypes.c_void_p(0x1000)


# ---------------------------------------------------------------- symbols
def test_nat_symbols_are_declared_and_exported(tmp_path):
    """nsx_csum.h declares the four calls and no _tuned twin (nsx_tune.h keeps its 16 declarations); the library
    exports them; the ABI version stays 2; the header says what the restatement needs; a plain C caller compiles
    against them and gets the documented codes."""
    inc = os.path.join(ROOT, "include")
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)  # noqa: E731
    decl = r"^int\s+(nsx_nat_[a-z_0-9]+)\("
    text = open(os.path.join(inc, "nsx_csum.h")).read()
    assert set(re.findall(decl, strip(text), flags=re.M)) == set(DEV_CALLS) | set(HOST_CALLS)
    for h in ("nsx_tune.h", "nsx_tx_tune.h", "nsx_gro_tune.h"):
        assert "nsx_nat_" not in strip(open(os.path.join(inc, h)).read()), h
    out = subprocess.run(["nm", "-D", "--defined-only", nsx.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (nsx_\w+)", out))
    assert set(DEV_CALLS) | set(HOST_CALLS) <= exported
    assert not [s for s in exported if s.startswith("nsx_nat_") and s.endswith("_tuned")]
    assert nsx.abi_version() == 2
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for word in ("0x811C9DC5", "0x01000193", "the same key that nsx_gro_flow_* defines", "RFC 1624",
                 "fold(x) = 0 if x = 0, else 1 + (x - 1) mod 0xFFFF", "State 1 means occupied",
                 "after slots probes the lookup is a miss", "total function of arbitrary table bytes",
                 "left byte for byte as it was", "IHL > 5) are translated like any other",
                 "stays wrong by the same one's-complement difference", "can be captured into a graph"):
        assert word in flat, word
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include <stdlib.h>
#include <string.h>
#include "nsx_csum.h"
int main(void) {
    uint64_t s = 0, offs[2] = {0, 0}, mask[1] = {0};
    if (nsx_nat_table_slots(0, &s) != NSX_OK || s != 16) return 1;
    if (nsx_nat_table_slots(8, &s) != NSX_OK || s != 16) return 2;
    if (nsx_nat_table_slots(9, &s) != NSX_OK || s != 32) return 3;
    if (nsx_nat_table_slots(1000, &s) != NSX_OK || s != 2048) return 4;
    if (nsx_nat_table_slots(1ull << 31, &s) != NSX_EINVAL || nsx_nat_table_slots(1, 0) != NSX_EINVAL) return 5;
    uint8_t m[24] = {1, 2, 3}, r[24] = {9}, *t = aligned_alloc(16, 16 * 32);
    memset(m + 12, 7, 12);
    if (nsx_nat_table_build_host(4, m, r, 2, t, 16) != NSX_OK) return 6;
    if (nsx_nat_table_build_host(5, m, r, 2, t, 16) != NSX_EINVAL) return 7;
    if (nsx_nat_table_build_host(4, m, r, 2, t, 8) != NSX_EINVAL) return 8;
    memcpy(m + 12, m, 12);
    if (nsx_nat_table_build_host(4, m, r, 2, t, 16) != NSX_EINVAL) return 9;
    if (nsx_nat_ipv4_tcp_rewrite_dev(offs, offs, 1, mask, t, 24, 0, mask, 0) != NSX_EINVAL) return 10;
    if (nsx_nat_ipv6_tcp_rewrite_dev(offs, offs, 1, mask, t, 16, 256, mask, 0) != NSX_EINVAL) return 11;
    if (nsx_nat_ipv4_tcp_rewrite_dev(offs, offs, 1, mask, t + 8, 16, 0, mask, 0) != NSX_EINVAL) return 12;
    free(t);
    return 0;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(nsx.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I", inc, "-L", libdir, "-lnsx_csum",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- validation
def _call(name, **kw):
    a = dict(base=fake, offsets=fake, n=100, valid=fake, table=fake, slots=16, ttl_dec=1, hit=fake)
    a.update(kw)
    return getattr(nsx.lib(), name)(a["base"], a["offsets"], a["n"], a["valid"], a["table"], a["slots"],
                                    a["ttl_dec"], a["hit"], None)


def test_nat_device_calls_validate_before_any_device_work():
    """NULL pointers, n >= 2^32 - 1, slots that are no power of two or exceed 2^31, a table off a 16-byte boundary and
    ttl_dec > 255 are NSX_EINVAL before anything else; a well-formed call on a host with no GPU is then NSX_ENODEV,
    n == 0 (where d_base, d_valid and d_hit may be NULL) included."""
    E = nsx.NSX_EINVAL
    for name in DEV_CALLS:
        for kw in (dict(base=None), dict(offsets=None), dict(valid=None), dict(table=None), dict(hit=None),
                   dict(n=0xFFFFFFFF), dict(n=1 << 32), dict(slots=0), dict(slots=3), dict(slots=24),
                   dict(slots=(1 << 31) + 1), dict(slots=1 << 32), dict(slots=1 << 63),
                   dict(table=ctypes.c_void_p(0x1008)), dict(table=ctypes.c_void_p(0x1001)), dict(ttl_dec=256),
                   dict(ttl_dec=0xFFFFFFFF), dict(n=0, offsets=None), dict(n=0, table=None), dict(n=0, slots=5)):
            assert _call(name, **kw) == E, kw
        if nsx.device_count() == 0:
            D = nsx.NSX_ENODEV
            assert _call(name) == D
            assert _call(name, ttl_dec=0) == D and _call(name, ttl_dec=255) == D
            assert _call(name, slots=1) == D and _call(name, slots=1 << 31) == D
            assert _call(name, n=0, base=None, valid=None, hit=None) == D
            assert _call(name, n=0xFFFFFFFE) == D


def test_nat_binding_checks_extents_before_the_c_call():
    """Every tensor is checked before the C call (CPU tensors here: a well-formed call is then refused as not on a
    device): valid and hit are 8-byte words, ceil(n/64) of them; table holds slots entries."""
    import torch
    n = 70
    offs = torch.arange(n + 1, dtype=torch.int64) * 60
    buf = torch.zeros(60 * n, dtype=torch.uint8)
    valid = torch.zeros(2, dtype=torch.int64)
    for ipver, fn in ((4, nsx.nat_ipv4_tcp_rewrite_dev), (6, nsx.nat_ipv6_tcp_rewrite_dev)):
        eb = nsx.NAT_ENTRY_BYTES[ipver]
        table = torch.zeros(16 * eb, dtype=torch.uint8)
        cases = [(dict(valid=valid[:1]), " valid"), (dict(valid=None), "`valid` is required"),
                 (dict(valid=torch.zeros(4, dtype=torch.int32)), "8-byte elements"),
                 (dict(hit=torch.zeros(1, dtype=torch.int64)), " hit"),
                 (dict(hit=torch.zeros(4, dtype=torch.int32)), "8-byte elements"),
                 (dict(table=table[:-1]), " table"), (dict(table=None), "`table` is required"),
                 (dict(slots=32), " table"), (dict(table=torch.zeros(32 * eb, dtype=torch.uint8)[::2]), "contiguous"),
                 (dict(offsets=offs.to(torch.int32)), "8-byte elements"),
                 (dict(buf=torch.zeros(60 * n, dtype=torch.int16)), "1-byte elements"),
                 (dict(ttl_dec=-1), "ttl_dec"), (dict(), "device")]
        for kw, msg in cases:
            args = dict(buf=buf, offsets=offs, valid=valid, table=table, slots=16, ttl_dec=1)
            args.update(kw)
            with pytest.raises(ValueError) as e:
                fn(**args)
            assert msg in str(e.value), (msg, str(e.value))
            assert f"nat_ipv{ipver}_tcp_rewrite_dev" in str(e.value) or msg == "device"


# ---------------------------------------------------------------- the table builder
def test_table_slots():
    for k, want in ((0, 16), (1, 16), (8, 16), (9, 32), (16, 32), (17, 64), (65536, 131072), (65537, 262144)):
        assert nsx.nat_table_slots(k) == want
    with pytest.raises(nsx.NsxError) as e:
        nsx.nat_table_slots(1 << 31)
    assert e.value.code == nsx.NSX_EINVAL


def _same_table(ipver, match, new, slots):
    got = nsx.nat_table_build_host(ipver, np.frombuffer(b"".join(match), np.uint8),
                                   np.frombuffer(b"".join(new), np.uint8), slots)
    want = _nat.build_table(ipver, match, new, slots)
    assert got.size == slots * nsx.NAT_ENTRY_BYTES[ipver] and np.array_equal(got, want)
    for m, r in zip(match, new):
        assert _nat.lookup(got, slots, m, ipver) == r
    return got


@pytest.mark.parametrize("ipver", [4, 6])
def test_table_build_matches_the_model(ipver):
    """Same bytes as tests/_nat.build_table: random rules at several loads; a chain of 5 colliding tuples (made with
    FL.ports_for_key) among random ones; a chain of 4 from the last slot, which wraps to slots 0-2; n_rules = 0."""
    rng = np.random.default_rng(0x4A7 + ipver)
    tb = _nat.TUPLE[ipver]
    for k, slots in ((0, 16), (1, 16), (8, 16), (9, 32), (300, 1024), (512, 1024)):
        _same_table(ipver, _nat.random_tuples(rng, k, ipver), _nat.random_tuples(rng, k, ipver), slots)
    assert not nsx.nat_table_build_host(ipver, np.zeros((0, tb), np.uint8), np.zeros((0, tb), np.uint8)).any()
    chain = _nat.chain_tuples(rng, ipver, 5, home=9, slots=64)
    match = _nat.random_tuples(rng, 6, ipver) + chain + _nat.random_tuples(rng, 6, ipver)
    t = _same_table(ipver, match, _nat.random_tuples(rng, len(match), ipver), 64)
    assert sum(_nat._entry(t, s, ipver)[0] for s in range(9, 14)) == 5
    wrap = _nat.chain_tuples(rng, ipver, 4, home=15, slots=16)
    t = _same_table(ipver, wrap, _nat.random_tuples(rng, 4, ipver), 16)
    assert [_nat._entry(t, s, ipver)[1] for s in (15, 0, 1, 2)] == wrap
    assert sum(_nat._entry(t, s, ipver)[0] for s in range(16)) == 4
    assert _nat.lookup(t, 16, _nat.chain_tuples(rng, ipver, 1, home=15, slots=16)[0], ipver) is None


@pytest.mark.parametrize("ipver", [4, 6])
def test_table_build_refusals(ipver):
    """Duplicate match tuples and bad slots are NSX_EINVAL, as are ip_ver 5 and NULL arrays with rules."""
    rng = np.random.default_rng(0x4B7 + ipver)
    m, r = _nat.random_tuples(rng, 9, ipver), _nat.random_tuples(rng, 9, ipver)
    cat = lambda ts: np.frombuffer(b"".join(ts), np.uint8)  # noqa: E731
    for slots in (0, 8, 16, 24, 31, 33):  # too small for 9 rules, or no power of two
        with pytest.raises(nsx.NsxError) as e:
            nsx.nat_table_build_host(ipver, cat(m), cat(r), slots)
        assert e.value.code == nsx.NSX_EINVAL, slots
        with pytest.raises(ValueError):
            _nat.build_table(ipver, m, r, slots)
    for dup in ([m[0]] + m[:8], m[:8] + [m[3]]):
        with pytest.raises(nsx.NsxError) as e:
            nsx.nat_table_build_host(ipver, cat(dup), cat(r), 32)
        assert e.value.code == nsx.NSX_EINVAL
        with pytest.raises(ValueError):
            _nat.build_table(ipver, dup, r, 32)
    nsx.nat_table_build_host(ipver, cat(m), cat([r[0]] * 9), 32)  # equal new tuples are no duplicates
    L, E = nsx.lib(), nsx.NSX_EINVAL
    table = np.zeros(32 * nsx.NAT_ENTRY_BYTES[ipver], np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert L.nsx_nat_table_build_host(5, p(cat(m)), p(cat(r)), 9, p(table), 32) == E
    assert L.nsx_nat_table_build_host(ipver, None, p(cat(r)), 9, p(table), 32) == E
    assert L.nsx_nat_table_build_host(ipver, p(cat(m)), None, 9, p(table), 32) == E
    assert L.nsx_nat_table_build_host(ipver, p(cat(m)), p(cat(r)), 9, None, 32) == E
    assert L.nsx_nat_table_build_host(ipver, None, None, 0, p(table), 8) == E
    assert L.nsx_nat_table_build_host(ipver, None, None, 0, p(table), 32) == 0
    with pytest.raises(ValueError):
        nsx.nat_table_build_host(ipver, cat(m)[:-1], cat(r))
    with pytest.raises(ValueError):
        nsx.nat_table_build_host(5, cat(m), cat(r))


# ---------------------------------------------------------------- the model, held to what exists
def test_lookup_is_total():
    """A table without an empty entry ends every lookup after `slots` probes: a miss for a tuple it does not hold, a
    hit for one it does; arbitrary bytes are a table too."""
    rng = np.random.default_rng(0x4C7)
    for ipver in (4, 6):
        eb, tb = _nat.ENTRY[ipver], _nat.TUPLE[ipver]
        full = np.zeros(16 * eb, np.uint8)
        held = _nat.random_tuples(rng, 16, ipver)
        for s, m in enumerate(held):
            full[s * eb:s * eb + tb] = np.frombuffer(m, np.uint8)
            full[s * eb + tb] = 1
        assert _nat.lookup(full, 16, _nat.random_tuples(rng, 1, ipver)[0], ipver) is None
        assert _nat.lookup(full, 16, held[5], ipver) == bytes(tb)
        junk = rng.integers(0, 256, 16 * eb, dtype=np.uint8)
        assert _nat.lookup(junk, 16, held[0], ipver) is None


def test_update_carry_edges():
    """Eqn. 3 by hand: fold's fixed points, a field of 0x0000, words of 0x0000 and 0xFFFF."""
    assert [_nat.fold(x) for x in (0, 1, 0xFFFF, 0x10000, 0x1FFFE, 0x1FFFF)] == [0, 1, 0xFFFF, 1, 0xFFFF, 1]
    assert _nat.update(0x0000, b"\x00\x00", b"\x00\x00") == 0x0000  # ~fold(0xFFFF + 0xFFFF + 0)
    assert _nat.update(0x1234, b"\xff\xff", b"\xff\xff") == 0x1234
    assert _nat.update(0x1234, b"\x00\x01", b"\x00\x02") == 0x1233
    assert _nat.update(0x0000, b"\x00\x02", b"\x00\x01") == 0x0001
    assert _nat.update(0xFFFF, b"\xff\xff", b"\x00\x00") == 0xFFFF  # the one input whose sum is 0


@pytest.mark.parametrize("opt", [False, True], ids=["noopt", "opt"])
@pytest.mark.parametrize("ttl_dec", [0, 1, 7])
@pytest.mark.parametrize("ipver", [4, 6])
def test_model_rewrite_is_the_transmit_model_on_the_new_fields(ipver, ttl_dec, opt):
    """Frames the transmit pass's model builds, every one in the table: rewritten by tests/_nat.rewrite they equal —
    padding and all — the frames tests/_tx.expected builds from the new addresses, ports and TTL, so the incremental
    update is the full recomputation on frames that verify."""
    rng = np.random.default_rng(0x4D7 + 16 * ipver + ttl_dec + 100 * opt)
    pays = [0, 1, 2, 3, 5, 100, 537, 1460, 0, 9]
    opts = [_tx.opt_bytes(rng, "mss") if i % 2 else b"" for i in range(len(pays))] if opt else None
    c = _tx.Case(rng, ipver, pays, opts=opts)
    c.ip["ttl"][:] = rng.integers(ttl_dec + 1, 256, c.n)
    c.ip["ttl"][0], c.ip["ttl"][1] = ttl_dec + 1, 255
    off = c.packed()
    buf, _ = _tx.expected(c, off, fill=0x5A)
    ends = off[:-1] + c.flen
    match = [_nat.tuple_of(buf[int(o):int(e)].tobytes(), ipver) for o, e in zip(off[:-1], ends)]
    new = _nat.random_tuples(rng, c.n, ipver)
    new[2] = match[2]  # a rule that changes nothing but the TTL
    new[3] = bytes(len(match[3])) if ipver == 4 else b"\xff" * len(match[3])
    slots = 32
    table = _nat.build_table(ipver, match, new, slots)
    # the frames sit in 4-aligned slots with zero padding: rewrite them one by one (the padding is no frame's)
    got = buf.copy()
    for i in range(c.n):
        o, e = int(off[i]), int(ends[i])
        one, hit = _nat.rewrite(buf[o:e], np.array([0, e - o], np.uint64), np.ones(1, bool), table, slots, ttl_dec,
                                ipver)
        assert hit.all()
        got[o:e] = one
    c2 = copy.deepcopy(c)
    alen = 4 if ipver == 4 else 16
    for i, t in enumerate(new):
        c2.ip["src"][i] = np.frombuffer(t[:alen], np.uint8)
        c2.ip["dst"][i] = np.frombuffer(t[alen:2 * alen], np.uint8)
        c2.fields["src_port"][i] = int.from_bytes(t[2 * alen:2 * alen + 2], "big")
        c2.fields["dst_port"][i] = int.from_bytes(t[2 * alen + 2:], "big")
    c2.ip["ttl"] = (c.ip["ttl"] - ttl_dec).astype(np.uint8)
    want, _ = _tx.expected(c2, off, fill=0x5A)
    assert np.array_equal(got, want)


def test_model_leaves_everything_else_alone():
    """Not translated: a clear valid bit, a malformed frame, TTL <= ttl_dec, a miss — the buffer is unchanged; a wrong
    TCP checksum stays wrong by the same difference."""
    rng = np.random.default_rng(0x4E7)
    for ipver in (4, 6):
        fr = _nat.frames(rng, ipver, [10, 11, 12, 13, 14], ttl=[9, 3, 2, 9, 9])
        match = [_nat.tuple_of(f, ipver) for f in fr[:4]]
        new = _nat.random_tuples(rng, 4, ipver)
        table = _nat.build_table(ipver, match, new, 16)
        ihl = 20 if ipver == 4 else 40
        bad = bytearray(fr[3])
        bad[ihl + 16] ^= 0x40  # frame 3: wrong TCP checksum, valid bit set all the same
        field = lambda f: int.from_bytes(f[ihl + 16:ihl + 18], "big")  # noqa: E731
        off_by = (field(bad) - field(fr[3])) % 0xFFFF
        fr[3] = bytes(bad)
        buf, offs = _nat.pack(fr, lead=1)
        valid = np.array([False, True, True, True, True])
        out, hit = _nat.rewrite(buf, offs, valid, table, 16, 2, ipver)
        assert hit.tolist() == [False, True, False, True, False]  # bit clear; ok; TTL 2 <= 2; ok; miss
        same = np.ones(buf.size, bool)
        for i in (1, 3):
            same[int(offs[i]):int(offs[i + 1])] = False
        assert np.array_equal(out[same], buf[same])
        f1 = out[int(offs[1]):int(offs[2])].tobytes()
        assert f1 == _gro.refix(f1, ipver) and _nat.tuple_of(f1, ipver) == new[1]
        f3 = out[int(offs[3]):int(offs[4])].tobytes()
        good = _gro.refix(f3, ipver)
        a, b = int.from_bytes(f3[ihl + 16:ihl + 18], "big"), int.from_bytes(good[ihl + 16:ihl + 18], "big")
        assert off_by != 0 and (a - b) % 0xFFFF == off_by
        assert f3[:ihl + 16] + good[ihl + 16:ihl + 18] + f3[ihl + 18:] == good  # nothing else differs
