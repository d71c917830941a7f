"""IPv4 fragmentation on the GPU (nsx_frag_ipv4_dev): every case compares the kernel with the numpy restatement
tests/_frag.py bit for bit — every output slot, the status array and the sentinel bytes around d_out (the output is
pre-filled with a fill byte) — at the smallest shapes at which the copy and the header fix-up can go wrong; then graph
capture and frames that lie past 2^32 in their arena."""
import numpy as np
import pytest

import _far
import _frag as F
import _frag_gpu as GPU
import _udp
from _gpu import host, setup_gpu, torch, nsx

pytestmark = pytest.mark.gpu

TUNES = (None, dict(blocks_per_cu=1))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    setup_gpu()


def _rng(*k):
    return np.random.default_rng([0xF6A0, *k])


def _payloads(mtu):
    """IP payload lengths whose last piece at this mtu is 1..8 bytes long and exactly per, over 2, 3 and 5 pieces."""
    per = F.per_of(mtu)
    return [k * per + r for k in (1, 2, 4) for r in (1, 2, 3, 4, 5, 6, 7, 8, per)]


@pytest.mark.parametrize("mtu", [28, 68, 576, 1500])
def test_cuts_with_every_short_last_piece(mtu):
    """Frames cut at mtu 28, 68, 576 and 1500 whose last piece is 1..8 bytes long and exactly per, between frames
    that fit (len == mtu among them) and one of len == mtu + 1; every fragment's header is valid."""
    rng = _rng(1, mtu)
    pays = [p - 8 for p in _payloads(mtu) if p >= 8] + [mtu - 28, mtu - 27, 0, 5]
    frames = F.udp_frames(rng, pays)
    if mtu == 28:
        # IP payloads shorter than a UDP header: any bytes behind a header that says their length
        frames += [_udp.set_len(np.frombuffer(frames[0][:20] + rng.integers(0, 256, k, dtype=np.uint8).tobytes(),
                                              np.uint8), 4, 20 + k).tobytes() for k in range(1, 10)]
    rng.shuffle(frames)
    buf, offs = F.pack(frames, lead=1)
    st, off, out = GPU.frag_check(buf, offs, mtu, TUNES, what=f"mtu={mtu}")
    assert set(st.tolist()) == {F.PASS, F.CUT} and (st == F.CUT).sum() >= 20
    for t in range(off.size - 1):
        s = out[int(off[t]):int(off[t + 1])]
        assert _udp.raw(s[:20]) == 0xFFFF, t


@pytest.mark.parametrize("leads", [range(0, 8), range(8, 16)], ids=lambda r: f"lead{r[0]}")
def test_short_pieces_at_every_source_and_destination_alignment(leads):
    """Pieces of 1..17, 31..33 and 48 bytes (mtu 68: per 48) and frames that pass, the batch behind 0..15 lead bytes and
    the output 0..15 bytes into its allocation: every source alignment against every destination alignment, with
    slots of every length meeting inside one dword."""
    mtu = 68
    pays = [48 * k + r for k in (1, 2) for r in list(range(1, 18)) + [31, 32, 33, 48]] + [0, 1, 2, 3, 30]
    for lead in leads:
        rng = _rng(2, lead)
        frames = F.udp_frames(rng, [max(p - 8, 0) for p in pays])
        buf, offs = F.pack(frames, lead=lead)
        GPU.frag_check(buf, offs, mtu, (None,), dleads=range(16), what=f"lead={lead}")


def test_long_pieces_cross_the_copy_row_pair():
    """A 9000-byte frame cut at mtu 4100 (pieces of 4080, 4080 and 820 bytes: two row pairs of the copy each), a
    65535-byte frame at the same mtu and at 1500, and a 9000-byte frame that passes at mtu 9000, at every fourth
    source and destination alignment."""
    rng = _rng(3)
    frames = F.udp_frames(rng, [8972, 65507, 8972, 100, 8973 - 8])
    mtu = np.array([4100, 4100, 9000, 4100, 1500], np.uint32)
    for lead in (0, 1, 6, 15):
        buf, offs = F.pack(frames, lead=lead)
        st, off, _ = GPU.frag_check(buf, offs, mtu, TUNES if lead == 0 else (None,), dleads=(0, 3, 9, 12),
                                    what=f"lead={lead}")
        assert st.tolist() == [F.CUT, F.CUT, F.PASS, F.PASS, F.CUT]
        assert np.diff(off)[:3].tolist() == [4100, 4100, 840]


def test_grid_takes_a_second_trip():
    """blocks_per_cu=1: one block (four wave tasks of 16 slots) per CU, so more than 64 slots per CU send every wave
    round its loop again."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = _rng(4)
    block = F.udp_frames(rng, [100, 30, 61, 0, 200, 41, 7, 120])
    n = 8 * (cus + 2) * 4 + 5
    frames = (block * (n // 8 + 1))[:n]
    buf, offs = F.pack(frames, lead=2)
    st, off, _ = GPU.frag_check(buf, offs, 68, (dict(blocks_per_cu=1), None))
    assert off.size - 1 > 64 * cus + 64


def test_mixed_statuses_zero_fill_and_sentinels():
    """Pass, cut, DF and bad frames — IHL 6, version 6, a total length that is not the frame's, an offset that would
    overflow — interleaved: the status array is the model's, the slots of DF and bad frames are zero (garbage-filled
    output to start with), and the sentinel bytes around d_out are unchanged."""
    rng = _rng(5)
    good = F.udp_frames(rng, [3000, 40, 1473, 2000])
    df = F.udp_frames(rng, [3000, 1500], df=True)
    base = good[0]
    ihl6 = bytearray(base[:20] + b"\x01\x01\x01\x00" + base[20:])
    ihl6[0] = 0x46
    ihl6 = _udp.set_len(np.frombuffer(bytes(ihl6), np.uint8), 4, len(ihl6)).tobytes()
    v6 = bytearray(base)
    v6[0] = 0x65
    mism = _udp.set_len(np.frombuffer(base, np.uint8), 4, len(base) - 1).tobytes()
    over = F.with_header(base, off=0x1FFF - 300)   # o*8 + len - 20 > 65535
    fits = F.with_header(base, off=(65535 - 3008) // 8)
    dfover = F.with_header(df[0], off=0x1FFF)
    junk = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    frames = [good[0], df[0], good[1], ihl6, bytes(v6), good[2], mism, over, fits, df[1], dfover, junk, good[3], b""]
    buf, offs = F.pack(frames, lead=3)
    st, off, out = GPU.frag_check(buf, offs, 1500, TUNES, dleads=(0, 5))
    assert st.tolist() == [F.CUT, F.DF, F.PASS, F.BAD, F.BAD, F.CUT, F.BAD, F.BAD, F.CUT, F.DF, F.BAD, F.BAD, F.CUT,
                           F.PASS]
    first = nsx.frag_count_host(offs, np.full(len(frames), 1500, np.uint32))
    for i in np.nonzero(st >= F.DF)[0]:
        assert not out[int(off[int(first[i])]):int(off[int(first[i + 1])])].any(), i
    # an mtu below 28, which only the device can see (the host helpers refuse it): status 3, the slot zero
    mtu = np.array([1500, 27, 1500], np.uint32)
    b3, o3 = F.pack([good[1], good[1], good[0]], lead=1)
    ok = np.array([1500, 1500, 1500], np.uint32)
    first, src, off = GPU.frag_map(o3, ok)
    arena = torch.full((int(off[-1]) + 128,), GPU.FILL, dtype=torch.uint8, device="cuda")
    status = nsx.frag_ipv4_dev(GPU.d(b3), GPU.d(o3), GPU.d(mtu), GPU.d(first), GPU.d(src), arena[64:], GPU.d(off))
    want, wst, _ = GPU.frag_want(b3, o3, ok)
    want[64:64 + len(good[1]) * 2][len(good[1]):] = 0
    assert host(status).tolist() == [F.PASS, F.BAD, F.CUT] and np.array_equal(host(arena), want)


def test_cutting_a_fragment_again_and_a_wrong_checksum():
    """A fragment (offset 185, MF set) cut again at mtu 576: the offsets add and the last piece keeps MF. A frame whose
    header checksum is wrong is cut all the same, and every fragment's field is wrong by the same difference."""
    rng = _rng(6)
    f = F.udp_frames(rng, [4000])[0]
    a, b, c = F.cut(f, 1500)
    bad = bytearray(f)
    bad[10] ^= 0x55
    frames = [b, c, a, bytes(bad)]
    buf, offs = F.pack(frames, lead=1)
    st, off, out = GPU.frag_check(buf, offs, 576, TUNES)
    assert st.tolist() == [F.CUT] * 4
    slots = [out[int(off[t]):int(off[t + 1])].tobytes() for t in range(off.size - 1)]
    assert [F.member(s) for s in slots[:3]] == [(185, 552, True), (254, 552, True), (323, 376, True)]
    assert [F.member(s) for s in slots[3:5]] == [(370, 552, True), (439, 496, False)]
    d = (F.be16(bad, 10) - F.be16(f, 10)) % 0xFFFF
    good_slots, _ = F.frag_frames([f], 576)
    for x, y in zip(slots[-len(good_slots):], good_slots):
        assert (F.be16(x, 10) - F.be16(y, 10)) % 0xFFFF == d and x[:10] == y[:10] and x[12:] == y[12:]


def test_device_call_captures_into_a_graph():
    """No allocation, no host sync: one call captured on a side stream, replayed twice into a re-filled output, gives the
    model's bytes both times."""
    rng = _rng(7)
    frames = F.udp_frames(rng, rng.integers(0, 4000, 300))
    buf, offs = F.pack(frames, lead=1)
    mtu = np.full(len(frames), 576, np.uint32)
    first, src, off = GPU.frag_map(offs, mtu)
    want, wst, _ = GPU.frag_want(buf, offs, mtu)
    args = [GPU.d(x) for x in (buf, offs, mtu, first, src)]
    d_off = GPU.d(off)
    arena = torch.full((want.size,), GPU.FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((len(frames),), GPU.FILL, dtype=torch.uint8, device="cuda")
    nsx.frag_ipv4_dev(*args, arena[GPU.GUARD:], d_off, status=status)  # a first call outside capture
    torch.cuda.synchronize()
    arena.fill_(GPU.FILL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        nsx.frag_ipv4_dev(*args, arena[GPU.GUARD:], d_off, status=status, tune=dict(blocks_per_cu=1))
    torch.cuda.synchronize()
    assert (host(arena) == GPU.FILL).all()  # capture ran nothing
    for _ in range(2):
        g.replay()
        assert np.array_equal(host(arena), want) and np.array_equal(host(status), wst)
        arena.fill_(GPU.FILL)
        status.fill_(GPU.FILL)
        torch.cuda.synchronize()


def test_frames_past_two_to_the_32():
    """The far frames of a 4 GiB arena (tests/_far.layout, a straddle placement: one frame lies across byte 2^32, every
    later one starts above it) are cut exactly as the same frames of the compact twin."""
    rng = _rng(8)
    near = F.udp_frames(rng, rng.integers(0, 200, 20))
    far = F.udp_frames(rng, [3000, 700] + [int(x) for x in rng.integers(0, 3000, 60)])
    head = bytes([0x45]) + rng.integers(0, 256, _far.HEAD - 1, dtype=np.uint8).tobytes()
    r = _far.layout(near, head, far, ("straddle", 1), lead=int(rng.integers(4)), rng=rng)
    k = r.span + 1
    cross = _far.crossing(r.far_offs)
    assert len(cross) == 1 and cross[0] >= k and int(r.far_offs[k]) < _far.TWO32 < int(r.far_offs[-1])
    arena = torch.zeros(_far.ARENA, dtype=torch.uint8, device="cuda")
    for dst, b in r.pieces():
        if len(b):
            arena[dst:dst + len(b)].copy_(torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()))
    twin_offs, far_offs = r.offs[k:].copy(), r.far_offs[k:].copy()
    want, wst, _ = GPU.frag_want(r.buf, twin_offs, 576)
    got, gst = GPU.frag_gpu(None, twin_offs, 576, d_buf=arena, d_offs=GPU.d(far_offs))
    del arena
    torch.cuda.empty_cache()
    assert np.array_equal(gst, wst) and (wst == F.CUT).sum() >= 20 and np.array_equal(got, want)
