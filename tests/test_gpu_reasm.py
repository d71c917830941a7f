"""IPv4 reassembly on the GPU (nsx_reasm_ipv4_dev): every case compares the kernels with the numpy restatement
tests/_frag.py bit for bit — every output array, the order, and the regions that must stay untouched (the outputs are
pre-filled with a fill byte) — at the smallest shapes at which each pass can go wrong; then the round trip transmit
pass → fragmentation → a device-side shuffle → reassembly → receive verify without the host, graph capture, and a
batch that lies past 2^32 in its arena."""
import numpy as np
import pytest

import _far
import _frag as F
import _frag_gpu as GPU
import _tx
import _udp
from _gpu import host, setup_gpu, torch, nsx

pytestmark = pytest.mark.gpu

SMALL = dict(run_segs=16, blocks_per_cu=1, rows=1)
TUNES = (None, SMALL)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    setup_gpu()


def _rng(*k):
    return np.random.default_rng([0xF6B0, *k])


def _pieces(rng, k, pay=8, tail=5, **hdr):
    """One datagram in k fragments: k - 1 of `pay` payload bytes and a last one of `tail`, cut by the model."""
    f = F.udp_frames(rng, [pay * (k - 1) + tail - 8])[0]
    if hdr:
        f = F.with_header(f, **hdr)
    fr = F.cut(f, 20 + pay) if k > 1 else [f]
    assert len(fr) == k
    return f, fr


# ---------------------------------------------------------------- head pass
@pytest.mark.parametrize("k", [2, 63, 64, 65])
def test_one_run_across_the_head_pass_wave_boundary(k):
    """A wave of the head pass owns 63 positions and reads the one before them in lane 0: a datagram of k fragments is
    one run whatever k is, in order, reversed, and behind another datagram that moves it across the boundary."""
    rng = _rng(1, k)
    f, fr = _pieces(rng, k)
    g, gr = _pieces(rng, 3)
    for frames in (fr, fr[::-1], gr + fr):
        buf, offs = F.pack(frames, lead=k % 4)
        o = GPU.reasm_check(buf, offs, TUNES, f"k={k}")
        assert f in F.datagrams(o) and k in o["frag_cnt"].tolist()


def test_runs_straddle_scan_block_edges():
    """run_segs=16: 330 fragments span 21 scan blocks. Datagrams of 1 (a leftover), 15, 16, 17, 31, 32, 33 and 5
    fragments in turn, all with one key (one ident), put first and last fragments and whole runs on either side of
    the block edges."""
    rng = _rng(2)
    frames, want = [], []
    src, dst = b"\x0a\x00\x00\x01", b"\x0a\x00\x00\x02"
    for r, k in enumerate((1, 15, 16, 17, 31, 32, 33, 5) * 3):
        f, fr = _pieces(rng, max(k, 2), src=src, dst=dst, ident=r, proto=17)
        frames += fr[:1] if k == 1 else fr
        want += [] if k == 1 else [f]
    frames = frames[:330]
    buf, offs = F.pack(frames, lead=2)
    o = GPU.reasm_check(buf, offs, TUNES)
    assert o["n_out"] >= 15 and o["frag_cnt"].tolist()[:7] != [] and set(F.datagrams(o)) <= set(want)
    # one key for everything: the same ident throughout, so every run breaks only where the offsets do
    frames = [F.with_header(x, ident=7) for x in frames]
    buf, offs = F.pack(frames, lead=1)
    GPU.reasm_check(buf, offs, TUNES, "one key")


# ---------------------------------------------------------------- the two sorts
def _with_key(f, key):
    """The fragment with its ident and protocol changed so that its key is `key`: FNV-1a's last step inverted."""
    inv = pow(0x01000193, -1, 1 << 32)
    h = 0x811C9DC5
    for w in (int.from_bytes(f[12:16], "little"), int.from_bytes(f[16:20], "little")):
        h = ((h ^ w) * 0x01000193) % (1 << 32)
    w = ((key * inv) % (1 << 32)) ^ h
    return w


@pytest.mark.parametrize("dist", ["equal", "distinct", "digit0", "digit1", "digit2", "digit3", "no_member"])
def test_several_sort_tiles_and_crafted_keys(dist):
    """rows=1: 256 keys per sort tile, so 600 frames span three. Key distributions: all equal (every datagram between
    one pair of hosts with one ident: the order is by offset then arrival, and only exact abutment joins), all
    distinct, one radix digit varying with the other three fixed, and no member at all. The third key dword holds only
    24 bits, so the addresses are searched for each key wanted."""
    rng = _rng(3, len(dist), ord(dist[-1]))
    nd = 200
    frames = []
    if dist == "no_member":
        frames = F.udp_frames(rng, rng.integers(0, 60, 600)) + [b"", b"\x45"]
    else:
        if dist == "equal":
            keys = None
        elif dist == "distinct":
            keys = [int(x) for x in rng.integers(0, 0xFFFFFFFF, nd)]
        else:
            sh = 8 * int(dist[-1])
            keys = [(0x5A6B7C8D & ~(0xFF << sh)) | (int(v) << sh) for v in rng.integers(0, 256, nd)]
        groups = []
        for r in range(nd):
            f, fr = _pieces(rng, 3, src=b"\x0a\x00\x00\x01", dst=b"\x0a\x00\x00\x02", ident=5, proto=17)
            if keys is not None:
                while True:  # a destination address under which some (ident, protocol) gives the key
                    d4 = rng.integers(0, 256, 4, dtype=np.uint8).tobytes()
                    w = _with_key(fr[0][:16] + d4, keys[r])
                    if w < 1 << 24:
                        break
                fr = [F.with_header(x, dst=d4, ident=((w & 0xFF) << 8) | ((w >> 8) & 0xFF), proto=w >> 16) for x in fr]
                assert {F.key(x) for x in fr} == {keys[r]}
            groups.append(fr)
        frames = [g[j] for j in range(3) for g in groups]  # interleaved: all first fragments, then all second, ...
    buf, offs = F.pack(frames, lead=1)
    o = GPU.reasm_check(buf, offs, (dict(rows=1), dict(rows=1, run_segs=16), None), dist)
    if dist == "distinct":
        assert o["n_out"] == nd and (o["frag_cnt"] == 3).all()
    if dist == "equal":  # 200 firsts, 200 middles, 200 lasts in the order: a run of two at each seam, none complete
        assert o["n_out"] == 0 and o["order"].tolist() == list(range(600))
    if dist == "no_member":
        assert o["n_out"] == 0 and not o["is_frag"].any() and o["order"].tolist() == list(range(len(frames)))


# ---------------------------------------------------------------- arrival orders
@pytest.mark.parametrize("how", ["reversed", "interleaved", "shuffled"])
def test_fragments_arrive_in_any_order(how):
    """300 datagrams of 2..9 fragments each, their fragments reversed, interleaved round-robin over all 300, and
    shuffled: every datagram comes back byte for byte."""
    rng = _rng(4, len(how))
    dgs, groups = [], []
    for r in range(300):
        f, fr = _pieces(rng, int(rng.integers(2, 10)), pay=8 * int(rng.integers(1, 9)), tail=int(rng.integers(1, 9)))
        dgs.append(f)
        groups.append(fr)
    if how == "reversed":
        frames = [x for g in groups for x in g[::-1]]
    elif how == "interleaved":
        frames = [g[j] for j in range(9) for g in groups if j < len(g)]
    else:
        frames = [x for g in groups for x in g]
        rng.shuffle(frames)
    buf, offs = F.pack(frames, lead=3)
    o = GPU.reasm_check(buf, offs, TUNES, how)
    assert o["n_out"] == 300 and sorted(F.datagrams(o)) == sorted(dgs)


# ---------------------------------------------------------------- broken runs
def test_duplicates_overlaps_gaps_and_leftovers():
    """A duplicate of the first, of a middle and of the last fragment; an overlap and a gap; a missing first and a
    missing last fragment (leftovers: is_frag set, frame_seg 0xFFFFFFFF); non-fragments and fragments with a wrong
    header checksum interleaved, neither of which is consumed; and the RFC 4963 mix of two datagrams with one ident.
    Outcomes are as the model says."""
    rng = _rng(5)
    frames, expect = [], 0
    for case in range(9):
        f = F.with_header(F.udp_frames(rng, [4000])[0], ident=case)
        a, b, c = F.cut(f, 1500)
        if case == 0:
            frames += [a, b, c, a]
            expect += 1
        elif case == 1:
            frames += [a, b, c, b]
        elif case == 2:
            frames += [c, a, b, c]
            expect += 1
        elif case == 3:
            frames += [a, F.with_header(b, off=184), c]  # overlaps a by 8 bytes
        elif case == 4:
            frames += [a, c]  # a gap
        elif case == 5:
            frames += [b, c]  # no first fragment
        elif case == 6:
            frames += [a, b]  # no last fragment
        elif case == 7:
            bad = bytearray(b)
            bad[8] ^= 1  # the TTL: the header checksum no longer holds
            frames += [a, bytes(bad), c, F.udp_frames(rng, [100])[0], F.tcp_frames(rng, [100])[0]]
        else:
            g = bytearray(F.udp_frames(rng, [4000])[0])
            g[4:20] = f[4:20]
            a2, b2, c2 = F.cut(F.with_header(bytes(g)), 1500)
            frames += [c, b2, a]  # what is left of two datagrams with one (src, dst, ident, protocol)
            expect += 1
    buf, offs = F.pack(frames, lead=1)
    o = GPU.reasm_check(buf, offs, TUNES)
    assert o["n_out"] == expect
    seg = o["frame_seg"]
    member = np.unpackbits(o["is_frag"].view(np.uint8), bitorder="little")[:len(frames)].astype(bool)
    assert member.sum() == len(frames) - 3 and (seg[~member] == F.NONE).all()
    assert ((seg == F.NONE) & member).sum() == 1 + 4 + 1 + 3 + 2 + 2 + 2 + 2  # the leftovers of cases 0..7


def test_a_65535_byte_datagram_from_mtu_1500_pieces():
    rng = _rng(6)
    f = F.udp_frames(rng, [65507])[0]
    fr = F.cut(f, 1500)
    assert len(f) == 65535 and len(fr) == 45
    rng.shuffle(fr)
    buf, offs = F.pack(fr + F.cut(F.udp_frames(rng, [20000])[0], 1500), lead=2)
    o = GPU.reasm_check(buf, offs, TUNES)
    assert o["n_out"] == 2 and f in F.datagrams(o)


def test_empty_batch_and_regions_past_n_out():
    """n == 0 writes *n_out = 0 and out_off[0] = 0 and nothing else, the order included; with datagrams, entries,
    offsets and bytes past the last one written are as they were (every comparison here is over worst-case arrays
    pre-filled with a fill byte)."""
    GPU.reasm_check(np.zeros(0, np.uint8), np.zeros(1, np.uint64), TUNES)
    rng = _rng(7)
    f, fr = _pieces(rng, 4)
    buf, offs = F.pack(fr + F.udp_frames(rng, [300, 0]) + _pieces(rng, 3)[1][:2], lead=1)
    w, o = GPU.reasm_want(buf, offs)
    assert o["n_out"] == 1 and (w["out"][len(f):] == GPU.FILL).all() and (w["first_pos"][1:].view(np.uint8) == GPU.FILL).all()
    GPU.reasm_same(GPU.reasm_gpu(buf, offs), w)


# ---------------------------------------------------------------- the round trip
@pytest.mark.parametrize("proto", ["udp", "tcp"])
def test_round_trip_transmit_frag_shuffle_reasm_verify(proto):
    """The transmit pass builds datagrams with payloads 1..20 000 (DF cleared on the device, the header checksum with
    it) → nsx_frag_ipv4_dev at mtu 1500 → a seeded device-side shuffle of the fragments → nsx_reasm_ipv4_dev → the
    receive verify over out / out_off: every mask bit is set, and the bytes equal the built datagrams. Nothing of the
    numpy model is used."""
    rng = _rng(8, len(proto))
    pays = [1, 2, 1471, 1472, 1473, 1480, 2952, 2953, 20000] + [int(x) for x in rng.integers(1, 20001, 40)]
    if proto == "udp":
        c = _udp.Case(rng, 4, pays)
        off = c.packed()
        built = torch.zeros(int(off[-1]), dtype=torch.uint8, device="cuda")
        nsx.udp_tx_ipv4_build_dev({k: GPU.d(v) for k, v in c.ip.items()}, {k: GPU.d(v) for k, v in c.ports.items()},
                                  GPU.d(c.data), GPU.d(c.data_off), built, GPU.d(off))
        verify = nsx.udp_rx_ipv4_verify_dev
    else:
        c = _tx.Case(rng, 4, pays)
        off = c.packed()
        built = torch.zeros(int(off[-1]), dtype=torch.uint8, device="cuda")
        nsx.tx_ipv4_tcp_build_dev({k: GPU.d(v) for k, v in c.ip.items()}, {k: GPU.d(v) for k, v in c.fields.items()},
                                  GPU.d(c.data), GPU.d(c.data_off), built, GPU.d(off))
        verify = nsx.rx_ipv4_tcp_verify_dev
    flen = np.asarray(c.flen, np.int64)
    n = len(pays)
    # the built datagrams packed densely, DF cleared: RFC 1624 by hand on the device (0x4000 leaves word 3)
    starts = torch.from_numpy(np.asarray(off[:-1], np.int64)).cuda()
    cs = (built[starts + 10].to(torch.int64) << 8) | built[starts + 11].to(torch.int64)
    x = (~cs & 0xFFFF) + (~torch.tensor(0x4000, device="cuda") & 0xFFFF)
    x = torch.where(x == 0, x, 1 + (x - 1) % 0xFFFF)
    cs = ~x & 0xFFFF
    built[starts + 6] = 0
    built[starts + 10] = (cs >> 8).to(torch.uint8)
    built[starts + 11] = (cs & 0xFF).to(torch.uint8)
    dense_off = np.zeros(n + 1, np.uint64)
    dense_off[1:] = np.cumsum(flen)
    idx = torch.cat([torch.arange(int(flen[i]), device="cuda") + int(off[i]) for i in range(n)])
    dense = built[idx].contiguous()
    mask = verify(dense, GPU.d(dense_off))
    assert int(host(mask).view(np.uint64)[0]) == (1 << 49) - 1, "the datagrams as built do not verify"
    # fragmentation
    mtu = np.full(n, 1500, np.uint32)
    first, src, foff = GPU.frag_map(dense_off, mtu)
    frags = torch.zeros(int(foff[-1]), dtype=torch.uint8, device="cuda")
    status = nsx.frag_ipv4_dev(dense, GPU.d(dense_off), GPU.d(mtu), GPU.d(first), GPU.d(src), frags, GPU.d(foff))
    want_st = np.where(flen > 1500, F.CUT, F.PASS)
    assert np.array_equal(host(status), want_st)
    # a seeded shuffle of the fragments on the device
    nf = src.size
    perm = np.random.default_rng(0x5EED).permutation(nf)
    slen = np.diff(foff).astype(np.int64)
    soff = np.zeros(nf + 1, np.uint64)
    soff[1:] = np.cumsum(slen[perm])
    gather = torch.cat([torch.arange(int(slen[t]), device="cuda") + int(foff[t]) for t in perm])
    shuffled = frags[gather].contiguous()
    for tune in TUNES:
        r = nsx.reasm_ipv4_dev(shuffled, GPU.d(soff), tune=tune)
        cut = np.nonzero(want_st == F.CUT)[0]
        assert int(r["n_out"].item()) == cut.size
        ns = cut.size
        out_off = r["out_off"][:ns + 1]
        mask = verify(r["out"], out_off)
        bits = np.unpackbits(host(mask).view(np.uint8), bitorder="little")[:ns]
        assert bits.all(), f"tune={tune}: {int((bits == 0).sum())} reassembled datagrams do not verify"
        d_host, oo, z = host(dense), host(out_off), host(r["out"])
        got = sorted(z[int(oo[s]):int(oo[s + 1])].tobytes() for s in range(ns))
        assert got == sorted(d_host[int(dense_off[i]):int(dense_off[i + 1])].tobytes() for i in cut)
        seg = host(r["frame_seg"][:nf]).view(np.uint32)
        passed = np.isin(src[perm], np.nonzero(want_st == F.PASS)[0])
        assert ((seg == F.NONE) == passed).all()


# ---------------------------------------------------------------- graph capture
def test_device_call_captures_into_a_graph():
    """No allocation, no host sync: one call captured on a side stream (a single chain of launches), replayed twice
    into re-filled outputs, gives the model's arrays both times."""
    rng = _rng(9)
    frames = []
    for r in range(60):
        frames += _pieces(rng, int(rng.integers(2, 8)))[1]
    frames += F.udp_frames(rng, [10, 200])
    rng.shuffle(frames)
    n = len(frames)
    buf, offs = F.pack(frames, lead=1)
    want, _ = GPU.reasm_want(buf, offs)
    d_buf, d_offs = GPU.d(buf), GPU.d(offs)
    nsx.reasm_ipv4_dev(d_buf, d_offs, tune=SMALL)  # a first call outside capture (library and device-info setup)
    torch.cuda.synchronize()
    out = GPU.filled(n, buf.size)
    order = out.pop("order")
    work = torch.empty(nsx.reasm_work_bytes(n), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        nsx.reasm_ipv4_dev(d_buf, d_offs, out=out, order=order, work=work, tune=SMALL)
    torch.cuda.synchronize()
    assert (host(out["frame_seg"]).view(np.uint8) == GPU.FILL).all()  # capture ran nothing
    for _ in range(2):
        g.replay()
        GPU.reasm_same(GPU.to_host(dict(out, order=order), n, buf.size), want, "replay")
        for t in list(out.values()) + [work, order]:
            t.view(torch.uint8).fill_(GPU.FILL)
        torch.cuda.synchronize()


# ---------------------------------------------------------------- far offsets
def test_frames_past_two_to_the_32():
    """A batch in a 4 GiB arena (tests/_far.layout, a straddle placement): near fragments, a span of almost 2^32 bytes
    which is no member, and far fragments of which one lies across byte 2^32 inside a complete run; datagrams whose
    fragments lie on both sides of the span. Every output array against the model on the compact twin; the output is
    given at its worst-case extent and nothing past the packed datagrams is written."""
    rng = _rng(10)
    groups = [_pieces(rng, int(rng.integers(2, 7)), pay=8 * int(rng.integers(1, 20)))[1] for _ in range(50)]
    near = [x for g in groups[:10] for x in g] + [g[0] for g in groups[10:20]]
    far = [x for g in groups[10:20] for x in g[1:]] + [x for g in groups[20:] for x in g]
    head = bytes([0x45]) + rng.integers(0, 256, _far.HEAD - 1, dtype=np.uint8).tobytes()
    r = _far.layout(near, head, far, ("straddle", 1), lead=int(rng.integers(4)), rng=rng)
    nb = r.buf.size
    w, o = GPU.reasm_want(r.buf, r.offs)
    cross = _far.crossing(r.far_offs)
    assert len(cross) == 1 and o["frame_seg"][r.span] == F.NONE and o["frame_seg"][cross[0]] != F.NONE
    assert o["n_out"] == 50 and nb <= 4 << 20
    arena = torch.zeros(_far.ARENA, dtype=torch.uint8, device="cuda")
    for dst, b in r.pieces():
        if len(b):
            arena[dst:dst + len(b)].copy_(torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()))
    out = GPU.filled(r.n, 1)
    order = out.pop("order")
    data = torch.empty(_far.ARENA, dtype=torch.uint8, device="cuda")
    data[:8 << 20] = GPU.FILL
    out["out"] = data
    res = nsx.reasm_ipv4_dev(arena, GPU.d(r.far_offs), out=out, order=order)
    got = {k: host(res[k][:nb] if k == "out" else res[k]).view(GPU._NP[dt]) for k, (dt, _) in GPU.sizes(r.n, nb).items()}
    ok = bool((data[nb:8 << 20] == GPU.FILL).all())
    del arena, data, out, res
    torch.cuda.empty_cache()
    GPU.reasm_same(got, w, "far")
    assert ok, "output bytes written past the twin's extent"
