"""The in-place echo reply on the GPU (nsx_icmp_echo_reply_ipv4_dev / nsx_icmp_echo_reply_ipv6_dev): the WHOLE buffer —
lead bytes, unanswered frames, neighbours and a guard region on either side of it, all over a fill byte — and the hit
words, bit-exact against the numpy restatement tests/_icmp.py (held to a rebuild from scratch by
tests/test_icmp_abi.py)."""
import numpy as np
import pytest

import _far
import _icmp as M
import _icmp_gen as G
import _icmp_gpu as GPU
from _gpu import dev, host, setup_gpu, torch, nsx
from _icmp_gpu import arena  # noqa: F401  (the module's 4 GiB fixture)

pytestmark = pytest.mark.gpu
d = GPU.d
KINDS = [(4, "minimal"), (4, "odd"), (4, "ihl6"), (4, "ihl15"), (6, "minimal"), (6, "odd")]
RQ = {4: 8, 6: 128}


def setup_module(module):
    setup_gpu()


def _rng(*key):
    return np.random.default_rng([0x1CE2, *key])


def _fn(ipver):
    return nsx.icmp_echo_reply_ipv4_dev if ipver == 4 else nsx.icmp_echo_reply_ipv6_dev


def _request(rng, ipver, data_len, ihl=5, **kw):
    data = rng.integers(0, 256, data_len, dtype=np.uint8).tobytes()
    if ipver == 4:
        kw["options"] = rng.integers(0, 256, 4 * (ihl - 5), dtype=np.uint8).tobytes()
    return G.icmp_frame(rng, ipver, RQ[ipver], 0, data, **kw)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("ipver,kind", KINDS, ids=[f"v{v}-{k}" for v, k in KINDS])
def test_packed_frames_at_every_alignment(ipver, kind, lead):
    """150 frames packed densely behind 0-3 lead bytes, the last one ending exactly at the buffer's end: minimal
    requests (28-byte IPv4, 48-byte IPv6: the ICMP checksum is 4 bytes from the neighbour), odd lengths (every
    alignment in one batch), IPv4 with IHL 6 and IHL 15. Two frames in three are requests; their neighbours —
    replies, other types — must not change."""
    rng = _rng(1, lead, ipver, len(kind))
    n = 150
    pays = np.zeros(n, int) if kind == "minimal" else rng.integers(0, 40, n) * 2 + 1 if kind == "odd" else \
        rng.integers(0, 9, n)
    ihl = int(kind[3:]) if kind.startswith("ihl") else 5
    fr = []
    for i in range(n):
        if i % 3 == 2:
            other = G.icmp_frame(rng, ipver, int(rng.choice([0, 13] if ipver == 4 else [129, 135])), 0, bytes(int(pays[i])))
            fr.append(other)
        else:
            fr.append(_request(rng, ipver, int(pays[i]), ihl))
    buf, offs = M.pack(fr, lead=lead, tail=0)
    assert int(offs[-1]) == buf.size
    hit = GPU.echo_check(buf, offs, np.ones(n, bool), 64, ipver, what=f"{kind} lead {lead}")
    assert np.array_equal(hit, np.arange(n) % 3 != 2)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 3000])
@pytest.mark.parametrize("ipver", [4, 6])
def test_frame_counts_across_wave_and_block_edges(ipver, n):
    """The hit words, the word past them included: bits past n are 0, no word past ceil(n/64) is written (n = 0 writes
    none), the last lanes of the last wave and block do their frames."""
    rng = _rng(2, n, ipver)
    fr = [_request(rng, ipver, int(rng.integers(0, 30))) for _ in range(n)]
    buf, offs = M.pack(fr, lead=n % 4)
    valid = rng.random(n) < 0.9
    valid[-1:] = True
    hit = GPU.echo_check(buf, offs, valid, 255, ipver, what=f"n {n}")
    assert np.array_equal(hit, valid)


@pytest.mark.parametrize("ttl", [0, 1, 255])
@pytest.mark.parametrize("ipver", [4, 6])
def test_ttl_and_carry_edges(ipver, ttl):
    """The new TTL 0, 1 and 255 over old TTLs of 0, 1, 128 and 255; requests whose ICMP checksum field is 0x0000 on
    entry and verifies, and 0xFFFF (a wrong one, which stays wrong); on IPv4, header checksum fields of 0x0000 that
    verify; identifier and sequence words of 0x0000 and 0xFFFF."""
    rng = _rng(3, ipver, ttl)
    fr = []
    for old in (0, 1, 128, 255):
        for rest in (bytes(4), b"\xff" * 4, b"\0\0\xff\xff"):
            data = rng.integers(0, 256, 10, dtype=np.uint8).tobytes()
            if ipver == 4:
                fr.append(M.ip4(1, GPU.B4, GPU.A4, M.icmp4(8, 0, rest, data), ttl=old))
            else:
                fr.append(M.ip6(58, GPU.B6, GPU.A6, M.icmp6(128, 0, rest, data, GPU.B6, GPU.A6), hop=old))
    # a checksum field of 0x0000 that verifies: the last data word takes the field's value up
    ihl = 20 if ipver == 4 else 40
    for f in list(fr[:4]):
        g = bytearray(f)
        field, word = int.from_bytes(g[ihl + 2:ihl + 4], "big"), int.from_bytes(g[-2:], "big")
        s = field + word
        g[-2:] = ((s & 0xFFFF) + (s >> 16)).to_bytes(2, "big")
        g[ihl + 2:ihl + 4] = b"\0\0"
        assert M.verify_frame(bytes(g), ipver)[0] or ipver == 4  # IPv4: the header checksum is still the old one
        fr.append(bytes(g))
        h = bytearray(f)
        h[ihl + 2:ihl + 4] = b"\xff\xff"
        fr.append(bytes(h))
    if ipver == 4:  # a header checksum field of 0x0000 that verifies: the ident takes it up
        for f in list(fr[:4]):
            g = bytearray(f)
            s = int.from_bytes(g[10:12], "big") + int.from_bytes(g[4:6], "big")
            g[4:6] = ((s & 0xFFFF) + (s >> 16)).to_bytes(2, "big")
            g[10:12] = b"\0\0"
            assert M.raw(g[:20]) == 0xFFFF
            fr.append(bytes(g))
    for lead in (0, 1):
        buf, offs = M.pack(fr, lead=lead)
        hit = GPU.echo_check(buf, offs, np.ones(len(fr), bool), ttl, ipver, what=f"ttl {ttl} lead {lead}")
        assert hit.all()


@pytest.mark.parametrize("ipver", [4, 6])
def test_frames_that_are_left_alone(ipver):
    """A clear valid bit over garbage and over a good request; set bits over a multicast dst, code 1, replies, other
    types, fragments, truncated and malformed frames of every kind of the verify: untouched byte for byte. A request
    with a wrong ICMP checksum (IPv4: or header checksum) under a set bit is answered and stays wrong by the same
    difference — the model's bytes."""
    rng = _rng(4, ipver)
    mc = bytes([224, 0, 0, 251]) if ipver == 4 else bytes([0xFF, 2] + [0] * 13 + [1])
    fr = [_request(rng, ipver, 20), rng.integers(0, 256, 90, dtype=np.uint8).tobytes(), _request(rng, ipver, 9, dst=mc),
          G.icmp_frame(rng, ipver, RQ[ipver], 1, bytes(8)), G.icmp_frame(rng, ipver, 0 if ipver == 4 else 129, 0, bytes(8))]
    fr += [G.rx_frame(rng, k, ipver, 60) for k in G.RX_KINDS[ipver] for _ in range(3)]
    wrong = []
    for at in ((2, 3) if ipver == 6 else (2, 3, -10, -11)):  # ICMP checksum bytes; IPv4 header bytes 10, 11
        g = bytearray(_request(rng, ipver, 15, ihl=7))
        ihl = (g[0] & 15) * 4 if ipver == 4 else 40
        g[ihl + at if at > 0 else -at] ^= 0x5A
        wrong.append(bytes(g))
    fr += wrong + [_request(rng, ipver, 33)]
    valid = np.ones(len(fr), bool)
    valid[:2] = False
    buf, offs = M.pack(fr, lead=3)
    hit = GPU.echo_check(buf, offs, valid, 64, ipver, what="left alone")
    k = len(fr) - len(wrong) - 1
    assert not hit[:5].any() and hit[k:].all()


@pytest.mark.parametrize("ipver", [4, 6])
def test_closed_loop_with_the_verify(ipver):
    """nsx_icmp_rx_*_verify_dev -> echo reply -> verify again without leaving the device: the mask after is the mask
    before, every answered frame's type word turns from request to reply, and the buffer equals the replies built
    from scratch."""
    buf, offs, _, _ = G.echo_batch(50, ipver)
    n = offs.size - 1
    rx = nsx.icmp_rx_ipv4_verify_dev if ipver == 4 else nsx.icmp_rx_ipv6_verify_dev
    d_buf, d_off = dev(buf), d(offs)
    t0, t1 = torch.zeros(n, dtype=torch.int16, device="cuda"), torch.zeros(n, dtype=torch.int16, device="cuda")
    before = rx(d_buf, d_off, type=t0).clone()
    hit = _fn(ipver)(d_buf, d_off, before, ttl=99)
    after = rx(d_buf, d_off, type=t1)
    v, h = GPU.bits_of(before, n), GPU.bits_of(hit, n)
    assert np.array_equal(host(after), host(before)) and 100 < h.sum() < v.sum()
    a, b = host(t0).view(np.uint16), host(t1).view(np.uint16)
    assert (a[h] == RQ[ipver] << 8).all() and (b[h] == (0 if ipver == 4 else 129 << 8)).all() and np.array_equal(a[~h], b[~h])
    fr = M.frames_of(buf, offs)
    want = buf.copy()
    for i in np.nonzero(h)[0]:
        want[int(offs[i]):int(offs[i + 1])] = np.frombuffer(M.rebuilt_reply(fr[i], 99, ipver), np.uint8)
    assert np.array_equal(host(d_buf), want)


@pytest.mark.parametrize("ipver", [4, 6])
def test_graph_capture_and_replay(ipver):
    """The call captured into a torch.cuda.graph runs nothing at capture and rewrites the buffer on replay."""
    buf, offs, valid, ttl = G.echo_batch(51, ipver)
    n = offs.size - 1
    want, whit, _ = GPU.echo_want(buf, offs, valid, ttl, ipver)
    arena_ = torch.full((GPU.GUARD + buf.size + GPU.GUARD,), GPU.FILL, dtype=torch.uint8, device="cuda")
    view = arena_[GPU.GUARD:GPU.GUARD + buf.size]
    view.copy_(dev(buf))
    d_offs, d_valid = d(offs), GPU.d_words(valid)
    hit = torch.full((8 * whit.size,), GPU.HIT_FILL, dtype=torch.uint8, device="cuda").view(torch.int64)
    _fn(ipver)(view.clone(), d_offs, d_valid, ttl=ttl)  # a first call outside capture, on a copy of the buffer
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _fn(ipver)(view, d_offs, d_valid, ttl=ttl, hit=hit)
    torch.cuda.synchronize()
    assert np.array_equal(host(view), buf) and (host(hit).view(np.uint8) == GPU.HIT_FILL).all()  # capture ran nothing
    g.replay()
    assert np.array_equal(host(arena_), want) and np.array_equal(host(hit).view(np.uint64), whit)


@pytest.mark.parametrize("placement", [("straddle", 1), ("wrap_frame", 0)], ids=_far.pid)
@pytest.mark.parametrize("ipver", [4, 6])
def test_frames_past_two_to_the_32(arena, ipver, placement):  # noqa: F811
    """A batch whose offsets pass 2^32 (tests/_far.layout): far requests are answered at their addresses above 2^32;
    the span's head is a request whose valid bit is set and stays as it is (the span is no well-formed frame: no length
    field says 2^32); nothing else in 4 GiB changes."""
    rng = _rng(5, ipver, _far.PLACEMENTS.index(placement))
    near = [_request(rng, ipver, int(rng.integers(0, 80))) for _ in range(150)]
    far = [_request(rng, ipver, int(rng.integers(0, 1400))) if rng.random() < 0.7 else
           G.rx_frame(rng, str(rng.choice(G.RX_KINDS[ipver])), ipver, 200) for _ in range(400)]
    f = _request(rng, ipver, 80)
    head = f + rng.integers(0, 256, _far.HEAD - len(f), dtype=np.uint8).tobytes()
    if placement[0] == "wrap_frame":
        placement = ("wrap_frame", len(f))
    r = _far.layout(near, head, far, placement, lead=int(rng.integers(4)), rng=rng)
    valid = rng.random(r.n) < 0.9
    valid[r.span] = True
    new, hit = M.echo(r.buf, r.offs, valid, 7, ipver)
    assert not hit[r.span] and hit[r.span + 1:].sum() > 150
    GPU.put(arena, r.pieces())
    d_hit = torch.full(((r.n + 63) // 64,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    _fn(ipver)(arena, d(r.far_offs), GPU.d_words(valid), ttl=7, hit=d_hit)
    assert np.array_equal(host(d_hit).view(np.uint64), GPU.words(hit))
    GPU.check_arena(arena, r.pieces(new), "echo")
