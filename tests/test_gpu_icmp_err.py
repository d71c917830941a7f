"""ICMP error generation and its request helpers on the GPU (nsx_icmp_err_ipv4_dev / nsx_icmp_err_ipv6_dev,
nsx_icmp_req_*): every output array — status, n_out, src_frame, out_off and the message bytes, each between guard
entries over a fill byte — bit-exact against the numpy restatement tests/_icmp.py (held to known answers and to the
existing models by tests/test_icmp_abi.py)."""
import numpy as np
import pytest

import _far
import _frag
import _gro
import _icmp as M
import _icmp_gen as G
import _icmp_gpu as GPU
import _nat
import _udp
from _gpu import host, setup_gpu, torch, nsx
from _icmp_gpu import arena  # noqa: F401  (the module's 4 GiB fixture)

pytestmark = pytest.mark.gpu
d = GPU.d
IPH = {4: 20, 6: 40}


def setup_module(module):
    setup_gpu()


def _rng(*key):
    return np.random.default_rng([0x1CE0, *key])


def _frame(rng, ipver, length, proto=17):
    """A frame of exactly `length` bytes (a whole IP header at the least) with a unicast source."""
    pay = rng.integers(0, 256, length - IPH[ipver], dtype=np.uint8).tobytes()
    src, dst = G._addr(rng, ipver), G._addr(rng, ipver)
    return M.ip4(proto, src, dst, pay) if ipver == 4 else M.ip6(proto, src, dst, pay)


def _reqs(rng, n, ipver):
    t = M.ALLOWED[ipver]
    return (np.array([int(t[i % len(t)]) | (i % 7) << 8 for i in range(n)], np.uint32),
            rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))


# ---------------------------------------------------------------- emit: alignment, the cap, the rows
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("ipver", [4, 6])
def test_short_quotes_at_every_source_and_destination_alignment(ipver, lead):
    """Quotes of 20..37 bytes (IPv6: 40..57), twice over, the batch behind 0..3 lead bytes and the output 0..15 bytes
    into its allocation: every source alignment against every destination alignment, the head that goes with the
    header 0..15 bytes long, messages of every length meeting inside one dword."""
    rng = _rng(1, ipver, lead)
    fr = [_frame(rng, ipver, IPH[ipver] + k % 18) for k in range(36)]
    buf, offs = M.pack(fr, lead=lead, tail=0)
    req, arg = _reqs(rng, len(fr), ipver)
    o = GPU.err_check(buf, offs, req, arg, ipver, dleads=range(16), what=f"short quotes lead {lead}", ident0=0xFFFE)
    assert o["n_out"] == 36 and sorted(set(np.diff(o["out_off"]))) == [M.HDR[ipver] + IPH[ipver] + k for k in range(18)]


@pytest.mark.parametrize("ipver", [4, 6])
def test_quotes_at_the_cap_and_either_side_of_it(ipver):
    """Frames of Q - 1, Q, Q + 1 and 2Q + 1 bytes (Q = 548 / 1232): the quote stops at the cap, odd and even, and the
    frame's bytes behind it are not summed; at every source alignment and five destination alignments."""
    rng = _rng(2, ipver)
    Q = M.QUOTE[ipver]
    fr = [_frame(rng, ipver, L) for L in (Q - 1, Q, Q + 1, 2 * Q + 1, Q - 2, Q, IPH[ipver], Q + 1)]
    req, arg = _reqs(rng, len(fr), ipver)
    for lead in range(4):
        buf, offs = M.pack(fr, lead=lead)
        o = GPU.err_check(buf, offs, req, arg, ipver, dleads=(0, 1, 7, 8, 15), what=f"cap lead {lead}")
        assert np.diff(o["out_off"]).max() == M.HDR[ipver] + Q


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_ipv6_quotes_across_the_row_boundary(lead):
    """IPv6 quotes of 1009..1056 bytes and the longest one: with a head of 0..15 bytes the wave's chunks end in the
    first 1 KiB row, exactly on its boundary and in the second row, at every alignment."""
    rng = _rng(3, lead)
    fr = [_frame(rng, 6, L) for L in list(range(1009, 1057, 3)) + [1232, 1024, 1025, 1039, 1040, 1041]]
    buf, offs = M.pack(fr, lead=lead)
    req, arg = _reqs(rng, len(fr), 6)
    GPU.err_check(buf, offs, req, arg, 6, dleads=range(16), what=f"row boundary lead {lead}")


def _with_field(f, ipver, want_raw):
    """Frame f (even length) with its last 16-bit word chosen so that the message's ICMP raw sum is want_raw."""
    g = bytearray(f)
    at = len(g) - 2
    assert at % 2 == 0 and at < M.QUOTE[ipver]
    g[at:at + 2] = b"\0\0"
    h = M.HDR[ipver]
    m0 = M.message(bytes(g), 3, 0, GPU.OUR[ipver], 64, 0, ipver)
    raw0 = ~int.from_bytes(m0[h - 6:h - 4], "big") & 0xFFFF
    x = (want_raw - raw0) % 0xFFFF  # one's-complement: raw0 + x folds to want_raw (1..0xFFFF)
    g[at:at + 2] = x.to_bytes(2, "big")
    return bytes(g)


@pytest.mark.parametrize("ipver", [4, 6])
def test_sums_that_fold_to_ffff_and_to_zero(ipver):
    """A message whose raw sum is 0xFFFF stores the field 0x0000 — ICMP has no 0 -> 0xFFFF rule — and one whose raw
    sum is 0x0001 stores 0xFFFE; quotes whose bytes behind the head are all 0xFF (every partial sum of the wave folds
    to 0xFFFF, one's-complement zero) and all zero (the partial sum is 0)."""
    rng = _rng(4, ipver)
    h = M.HDR[ipver]
    fr = []
    for L in (IPH[ipver] + 12, IPH[ipver] + 200, 500):
        fr += [_with_field(_frame(rng, ipver, L), ipver, 0xFFFF), _with_field(_frame(rng, ipver, L), ipver, 1)]
    for byte in (0xFF, 0x00):
        for L in (IPH[ipver] + 41, 300):
            f = bytearray(_frame(rng, ipver, L))
            f[IPH[ipver]:] = bytes([byte]) * (L - IPH[ipver])
            fr.append(bytes(f))
    req = np.full(len(fr), 3, np.uint32)
    for lead in (0, 1):
        buf, offs = M.pack(fr, lead=lead)
        o = GPU.err_check(buf, offs, req, None, ipver, dleads=(0, 3, 6, 9), what=f"folds lead {lead}")
        fields = [int.from_bytes(m[h - 6:h - 4], "big") for m in o["msgs"]]
        assert fields[:6] == [0x0000, 0xFFFE] * 3


@pytest.mark.parametrize("ipver", [4, 6])
def test_emit_grid_takes_a_second_trip(ipver):
    """blocks_per_cu=1: one block (four wave tasks of 16 messages) per CU, so more than 64 messages per CU send every
    wave round its loop again; the last group is ragged."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * cus + 150
    rng = _rng(5, ipver)
    tmpl = [_frame(rng, ipver, IPH[ipver] + k) for k in range(9)]
    fr = [tmpl[int(k)] for k in rng.integers(0, 9, n)]
    buf, offs = M.pack(fr, lead=1)
    req, arg = _reqs(rng, n, ipver)
    o = GPU.err_check(buf, offs, req, arg, ipver, tunes=(dict(blocks_per_cu=1),), dleads=(5,), what="second trip",
                      ident0=0xFFF0)
    assert o["n_out"] == n


# ---------------------------------------------------------------- plan and scan
def _edge_frames(rng, ipver):
    """Frames of 0, 19 / 20 and 39 / 40 bytes, an ICMP frame with and without its type byte, and one of every kind of
    tests/_icmp_gen.py."""
    fr = [b"", _frame(rng, 4, 20)[:19], _frame(rng, 4, 20), _frame(rng, 6, 40)[:39], _frame(rng, 6, 40),
          _frame(rng, ipver, IPH[ipver] + 1), _frame(rng, ipver, IPH[ipver], proto=1 if ipver == 4 else 58),
          _frame(rng, ipver, IPH[ipver] + 1, proto=1 if ipver == 4 else 58),
          G.icmp_frame(rng, ipver, 8 if ipver == 4 else 128), G.icmp_frame(rng, ipver, 3 if ipver == 4 else 1)]
    return fr + [G.err_frame(rng, k, ipver) for k in G.ERR_KINDS]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("ipver", [4, 6])
def test_frame_counts_across_wave_and_block_edges(ipver, n):
    """63, 64 and 65 frames, a block and one more, one frame and none (n == 0 writes *n_out = 0 and out_off[0] = 0 and
    nothing else), each with the default scan block and with run_segs = 16; the frames are of every kind, a quarter
    of the requests zero and a tenth refused."""
    rng = _rng(6, ipver, n)
    pool = _edge_frames(rng, ipver)
    fr = [pool[int(k)] for k in rng.integers(0, len(pool), n)]
    buf, offs = M.pack(fr, lead=n % 4)
    req, arg = G.requests(rng, n, ipver)
    o = GPU.err_check(buf, offs, req, arg, ipver, tunes=(None, dict(run_segs=16)), what=f"n {n}", ident0=n)
    if n == 0:
        assert o["n_out"] == 0 and o["out_off"].tolist() == [0]


def _mixed(rng, ipver, n):
    pool = _edge_frames(rng, ipver) + [_frame(rng, ipver, L) for L in (60, 61, 700, 1500)]
    fr = [pool[int(k)] for k in rng.integers(0, len(pool), n)]
    req, arg = G.requests(rng, n, ipver)
    pre = np.array([M.pre_status(f, int(r), ipver) for f, r in zip(fr, req)])
    assert all((pre == s).sum() > n // 50 for s in (M.NONE, M.SENT, M.QUIET, M.BAD))
    return fr, req, arg, int((pre == M.SENT).sum())


@pytest.mark.parametrize("ipver", [4, 6])
def test_batch_across_scan_blocks(ipver):
    """4500 frames of every kind over run_segs = 16 (282 scan blocks: the sums kernel takes a second trip), 17 and the
    default, all five statuses mixed over sentinel-filled outputs, the ident wrapping from 0xFFFE."""
    rng = _rng(7, ipver)
    fr, req, arg, eligible = _mixed(rng, ipver, 4500)
    buf, offs = M.pack(fr, lead=3)
    o = GPU.err_check(buf, offs, req, arg, ipver, tunes=(dict(run_segs=16), dict(run_segs=17, blocks_per_cu=2), None),
                      what="scan blocks", max_out=eligible // 2, ident0=0xFFFE, ttl=255)
    assert np.bincount(o["status"], minlength=5).min() > 90


@pytest.mark.parametrize("ipver", [4, 6])
def test_every_cap(ipver):
    """max_out of 0, 1, exactly the eligible count, one less, one more and 2^40 over 600 mixed frames; the outputs are
    sized for each cap as the header comment's worst case says, with a guard entry behind each."""
    rng = _rng(14, ipver)
    fr, req, arg, eligible = _mixed(rng, ipver, 600)
    buf, offs = M.pack(fr, lead=1)
    for cap in (0, 1, eligible, eligible - 1, eligible + 1, 1 << 40):
        o = GPU.err_check(buf, offs, req, None, ipver, tunes=(dict(run_segs=64),), what=f"max_out {cap}", max_out=cap)
        assert o["n_out"] == min(cap, eligible) and (o["status"] == M.LIMITED).sum() == max(eligible - cap, 0)


@pytest.mark.parametrize("ipver", [4, 6])
def test_zero_requests_read_nothing(ipver):
    """Frames whose request is 0 lie over garbage behind the batch's defined part — inside the allocation, past
    everything the test wrote a frame into — with lengths no pass could take: their status is NONE and nothing else
    is written for them, whatever the bytes say; the refused request words (unknown types, high bits) do not read
    their frames either."""
    rng = _rng(8, ipver)
    fr = [_frame(rng, ipver, L) for L in (IPH[ipver], 77, 300)] * 5
    buf, offs = M.pack(fr, lead=2, tail=0)
    junk = rng.integers(0, 256, 3000, dtype=np.uint8)
    junk[0] = 0x45 if ipver == 4 else 0x60  # it would parse as a header if it were read
    buf2 = np.concatenate([buf, junk])
    ends = int(offs[-1]) + np.array([0, 1, 20, 60, 1500, 2999, 3000], np.uint64)
    offs2 = np.concatenate([offs, ends[1:]])
    n = offs2.size - 1
    req = np.zeros(n, np.uint32)
    req[:len(fr)] = _reqs(rng, len(fr), ipver)[0]
    req[len(fr) + 1] = 5          # a refused type over garbage: BAD without a read
    req[len(fr) + 3] = 3 | 1 << 20  # high bits
    o = GPU.err_check(buf2, offs2, req, None, ipver, what="zero requests")
    assert o["status"][len(fr):].tolist() == [M.NONE, M.BAD, M.NONE, M.BAD, M.NONE, M.NONE] and o["n_out"] == len(fr)


# ---------------------------------------------------------------- request helpers
def test_req_frag_writes_only_where_the_status_is_df():
    """Statuses 0..3 and junk values, sentinel-filled req / arg with a guard entry: only the DF entries change; n = 0
    launches nothing."""
    rng = _rng(9)
    for n in (0, 1, 255, 256, 257, 3000):
        status = rng.choice([0, 1, 2, 3, 2, 0xAB], n).astype(np.uint8)
        mtu = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        req0 = rng.integers(0, 1 << 32, n + 1, dtype=np.uint64).astype(np.uint32)
        arg0 = rng.integers(0, 1 << 32, n + 1, dtype=np.uint64).astype(np.uint32)
        d_req, d_arg = d(req0), d(arg0)
        nsx.icmp_req_frag_dev(d(status) if n else torch.zeros(1, dtype=torch.uint8, device="cuda"),
                              d(mtu) if n else torch.zeros(1, dtype=torch.int32, device="cuda"), d_req[:n], d_arg[:n])
        wreq, warg = M.req_frag(status, mtu, req0[:n], arg0[:n])
        assert np.array_equal(host(d_req).view(np.uint32), np.concatenate([wreq, req0[n:]])), n
        assert np.array_equal(host(d_arg).view(np.uint32), np.concatenate([warg, arg0[n:]])), n


@pytest.mark.parametrize("ttl_dec", [0, 1, 255])
@pytest.mark.parametrize("ipver", [4, 6])
def test_req_ttl_edges(ipver, ttl_dec):
    """TTL / hop limit equal to ttl_dec, one more, 0, 1 and 255 over frames of every kind of the error generator
    (short and malformed ones among them), a random valid mask: only entries whose bit is set, whose frame holds a
    whole header and whose TTL is <= ttl_dec change; the guard entries stay."""
    rng = _rng(10, ipver, ttl_dec)
    n = 700
    fr = []
    for i in range(n):
        f = bytearray(G.err_frame(rng, str(rng.choice(G.ERR_KINDS)), ipver, 100))
        if len(f) > 8:
            f[8 if ipver == 4 else 7] = int(rng.choice([ttl_dec, min(ttl_dec + 1, 255), 0, 1, 255, 64]))
        fr.append(bytes(f))
    buf, offs = M.pack(fr, lead=int(rng.integers(4)))
    valid = rng.random(n) < 0.8
    req0 = np.zeros(n + 1, np.uint32)
    arg0 = np.full(n + 1, 0xDEADBEEF, np.uint32)
    req0[::7] = 0x0403
    d_req, d_arg = d(req0), d(arg0)
    fn = nsx.icmp_req_ttl_ipv4_dev if ipver == 4 else nsx.icmp_req_ttl_ipv6_dev
    fn(d(buf), d(offs), GPU.d_words(valid), ttl_dec, d_req[:n], d_arg[:n])
    wreq, warg = M.req_ttl(buf, offs, valid, ttl_dec, req0[:n], arg0[:n], ipver)
    hits = (wreq == (11 if ipver == 4 else 3)).sum()
    assert 20 < hits < n and (warg == 0).sum() == hits
    assert np.array_equal(host(d_req).view(np.uint32), np.concatenate([wreq, req0[n:]]))
    assert np.array_equal(host(d_arg).view(np.uint32), np.concatenate([warg, arg0[n:]]))


# ---------------------------------------------------------------- closed loops on the device
def test_closed_loop_udp_tx_frag_df_errors_verify():
    """nsx_udp_tx_ipv4_build_dev -> nsx_frag_ipv4_dev with mtu 576 (every datagram has DF set: all status 2) ->
    nsx_icmp_req_frag_dev -> nsx_icmp_err_ipv4_dev -> nsx_icmp_rx_ipv4_verify_dev without leaving the device: every
    message verifies, its type word is 0x0304, its next-hop MTU 576 and its quote the datagram's first 548 bytes."""
    rng = _rng(11)
    n = 300
    c = _udp.Case(rng, 4, rng.integers(140, 360, n) * 4)  # 588..1468-byte frames in dense 4-aligned slots
    c.ip["src"][:, 0] = rng.integers(1, 224, n)  # unicast on both sides: no datagram is one to stay quiet about
    c.ip["dst"][:, 0] = rng.integers(1, 224, n)
    off = c.packed()
    assert np.array_equal(np.diff(off), c.flen) and c.flen.min() > 576
    built = torch.full((int(off[-1]),), GPU.FILL, dtype=torch.uint8, device="cuda")
    nsx.udp_tx_ipv4_build_dev({k: d(v.reshape(-1)) for k, v in c.ip.items()}, {k: d(v) for k, v in c.ports.items()},
                              d(c.data), d(c.data_off), built, d(off))
    mtu = np.full(n, 576, np.uint32)
    first = nsx.frag_count_host(off, mtu)
    fsrc, foff = nsx.frag_layout_host(off, mtu, first)
    slots = torch.full((int(foff[-1]),), GPU.FILL, dtype=torch.uint8, device="cuda")
    d_mtu, d_off = d(mtu), d(off)
    status = nsx.frag_ipv4_dev(built, d_off, d_mtu, d(first), d(fsrc), slots, d(foff))
    req, arg = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    nsx.icmp_req_frag_dev(status, d_mtu, req, arg)
    res = nsx.icmp_err_ipv4_dev(built, d_off, req, GPU.A4, arg=arg, ttl=64, ident0=7)
    typ = torch.zeros(n, dtype=torch.int16, device="cuda")
    mask = nsx.icmp_rx_ipv4_verify_dev(res["out"], res["out_off"][:n + 1], type=typ)
    assert (host(status)[:n] == _frag.DF).all() and int(res["n_out"].item()) == n
    assert GPU.bits_of(mask, n).all() and (host(typ).view(np.uint16) == 0x0304).all()
    frames, oo, out = host(built), host(res["out_off"]).view(np.uint64), host(res["out"])
    for s in (0, 1, n - 1):
        m = out[int(oo[s]):int(oo[s + 1])].tobytes()
        assert m[24:28] == (576).to_bytes(4, "big") and m[28:] == frames[int(off[s]):int(off[s]) + 548].tobytes()
        assert m[16:20] == c.ip["src"][s].tobytes() and m[12:16] == GPU.A4


@pytest.mark.parametrize("ipver", [4, 6])
def test_closed_loop_nat_ttl_errors_verify(ipver):
    """Verified TCP frames -> the NAT rewrite with ttl_dec = 3 (every tuple has a rule: the frames it refuses are
    exactly those whose TTL is <= 3) -> nsx_icmp_req_ttl_* over the same mask -> errors -> verify: a request for every
    verified frame the rewrite refused and for no other, every message verifies as "time exceeded"."""
    rng = _rng(12, ipver)
    n, dec = 400, 3
    fr = _nat.frames(rng, ipver, rng.integers(0, 700, n), ttl=rng.integers(0, 8, n))
    sa, da = (12, 16) if ipver == 4 else (8, 24)
    for k, f in enumerate(fr):  # unicast on both sides (no frame is one to stay quiet about), checksums redone
        g = bytearray(f)
        g[sa], g[da] = int(rng.integers(1, 224)), int(rng.integers(1, 224))
        fr[k] = _gro.refix(bytes(g), ipver)
    broken = np.arange(n) % 9 == 0
    fr = [f[:-1] + bytes([f[-1] ^ 0x55]) if b else f for f, b in zip(fr, broken)]
    buf, offs = _nat.pack(fr, lead=1)
    match = list(dict.fromkeys(_nat.tuple_of(f, ipver) for f in fr))
    slots = nsx.nat_table_slots(len(match))
    table = _nat.build_table(ipver, match, _nat.random_tuples(rng, len(match), ipver), slots)
    rx = nsx.rx_ipv4_tcp_verify_dev if ipver == 4 else nsx.rx_ipv6_tcp_verify_dev
    nat = nsx.nat_ipv4_tcp_rewrite_dev if ipver == 4 else nsx.nat_ipv6_tcp_rewrite_dev
    rt = nsx.icmp_req_ttl_ipv4_dev if ipver == 4 else nsx.icmp_req_ttl_ipv6_dev
    err = nsx.icmp_err_ipv4_dev if ipver == 4 else nsx.icmp_err_ipv6_dev
    vfy = nsx.icmp_rx_ipv4_verify_dev if ipver == 4 else nsx.icmp_rx_ipv6_verify_dev
    d_buf, d_off = d(buf), d(offs)
    valid = rx(d_buf, d_off)
    req, arg = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    rt(d_buf, d_off, valid, dec, req, arg)  # before the rewrite changes the TTLs
    hit = nat(d_buf, d_off, valid, d(table), slots, ttl_dec=dec)
    res = err(d_buf, d_off, req, GPU.OUR[ipver], arg=arg)
    v, h = GPU.bits_of(valid, n), GPU.bits_of(hit, n)
    greq = host(req).view(np.uint32)
    assert np.array_equal(v, ~broken) and np.array_equal(greq != 0, v & ~h) and 50 < (greq != 0).sum() < n
    k = int(res["n_out"].item())
    ttls = np.array([f[8 if ipver == 4 else 7] for f in fr])
    assert k == (v & (ttls <= dec)).sum()  # every source is unicast and no frame is ICMP: none is QUIET
    typ = torch.zeros(k, dtype=torch.int16, device="cuda")
    mask = vfy(res["out"], res["out_off"][:k + 1], type=typ)
    assert GPU.bits_of(mask, k).all() and (host(typ).view(np.uint16) == (0x0B00 if ipver == 4 else 0x0300)).all()


# ---------------------------------------------------------------- graph capture, far offsets
@pytest.mark.parametrize("ipver", [4, 6])
def test_graph_capture_and_replay(ipver):
    """The call captured into a torch.cuda.graph runs nothing at capture and gives the model's outputs on each of two
    replays into re-filled outputs."""
    buf, offs, req, arg, kw = G.err_batch(0, ipver)
    n = offs.size - 1
    w, o = GPU.err_want(buf, offs, req, arg, ipver, **kw)
    cnt, ob = GPU.err_sizes(n, kw["max_out"], ipver, buf.size)
    t = dict(n_out=GPU.filled(cnt["n_out"], torch.int64), out_off=GPU.filled(cnt["out_off"], torch.int64),
             src_frame=GPU.filled(cnt["src_frame"], torch.int32), status=GPU.filled(cnt["status"], torch.uint8))
    out = torch.full((GPU.GUARD + ob + GPU.GUARD,), GPU.FILL, dtype=torch.uint8, device="cuda")
    outs = dict(t, out=out[GPU.GUARD:])
    fn = nsx.icmp_err_ipv4_dev if ipver == 4 else nsx.icmp_err_ipv6_dev
    args = (d(buf), d(offs), d(req), kw["src"])
    ckw = dict(arg=None if arg is None else d(arg), ttl=kw["ttl"], ident0=kw["ident0"], max_out=kw["max_out"])
    work = torch.empty(nsx.icmp_err_work_bytes(n), dtype=torch.uint8, device="cuda")
    fn(*args, **ckw, work=work)  # a first call outside capture (library and device-info setup), into its own outputs
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn(*args, **ckw, out=outs, work=work, tune=dict(run_segs=64, blocks_per_cu=1))
    torch.cuda.synchronize()
    assert (host(out) == GPU.FILL).all() and (host(t["status"]) == GPU.FILL).all()  # capture ran nothing
    for _ in range(2):
        g.replay()
        got = {k: host(t[k]).view(GPU._DT[k]) for k in t}
        got["out"] = host(out)
        GPU.err_same(got, w, o, "graph replay")
        for x in list(t.values()) + [out]:
            x.view(torch.uint8).fill_(GPU.FILL)
        torch.cuda.synchronize()


@pytest.mark.parametrize("ipver", [4, 6])
def test_request_helpers_errors_and_verify_as_one_graph(ipver):
    """What the helpers are for: zeroing the request arrays, nsx_icmp_req_frag_dev (IPv4), nsx_icmp_req_ttl_*_dev, the
    error call and the verify of its messages captured into one torch.cuda.graph. Capture runs nothing; each of two
    replays gives the model's request words, the model's error outputs and a set bit for every message."""
    rng = _rng(15, ipver)
    n, dec = 500, 2
    fr = []
    for i in range(n):
        f = bytearray(_frame(rng, ipver, IPH[ipver] + int(rng.integers(0, 900))))
        f[8 if ipver == 4 else 7] = int(rng.integers(0, 6))  # TTL / hop limit (no pass here looks at the header checksum)
        fr.append(bytes(f))
    buf, offs = M.pack(fr, lead=2)
    status = rng.choice([0, 1, 2, 3], n).astype(np.uint8) if ipver == 4 else np.zeros(n, np.uint8)
    mtu = rng.choice([576, 1280, 1500, 0x10000 | 68], n).astype(np.uint32)
    valid = rng.random(n) < 0.8
    wreq, warg = M.req_frag(status, mtu, np.zeros(n, np.uint32), np.zeros(n, np.uint32))
    wreq, warg = M.req_ttl(buf, offs, valid, dec, wreq, warg, ipver)
    kw = dict(ident0=0xFFFD, max_out=n // 3, ttl=9)
    w, o = GPU.err_want(buf, offs, wreq, warg, ipver, **kw)
    k = o["n_out"]
    assert k == n // 3 and (o["status"] == M.LIMITED).sum() > 10 and (wreq == 0).sum() > 50
    cnt, ob = GPU.err_sizes(n, kw["max_out"], ipver, buf.size)
    t = dict(n_out=GPU.filled(cnt["n_out"], torch.int64), out_off=GPU.filled(cnt["out_off"], torch.int64),
             src_frame=GPU.filled(cnt["src_frame"], torch.int32), status=GPU.filled(cnt["status"], torch.uint8))
    out = torch.full((GPU.GUARD + ob + GPU.GUARD,), GPU.FILL, dtype=torch.uint8, device="cuda")
    outs = dict(t, out=out[GPU.GUARD:])
    d_buf, d_offs, d_status, d_mtu, d_valid = d(buf), d(offs), d(status), d(mtu), GPU.d_words(valid)
    req, arg = GPU.filled(n, torch.int32), GPU.filled(n, torch.int32)
    mask, typ = GPU.filled((k + 63) // 64, torch.int64), GPU.filled(k, torch.int16)
    work = torch.empty(nsx.icmp_err_work_bytes(n), dtype=torch.uint8, device="cuda")
    err = nsx.icmp_err_ipv4_dev if ipver == 4 else nsx.icmp_err_ipv6_dev
    rt = nsx.icmp_req_ttl_ipv4_dev if ipver == 4 else nsx.icmp_req_ttl_ipv6_dev
    vfy = nsx.icmp_rx_ipv4_verify_dev if ipver == 4 else nsx.icmp_rx_ipv6_verify_dev

    def chain(req, arg, outs, mask, typ):
        req.zero_()
        arg.zero_()
        if ipver == 4:
            nsx.icmp_req_frag_dev(d_status, d_mtu, req, arg)
        rt(d_buf, d_offs, d_valid, dec, req, arg)
        res = err(d_buf, d_offs, req, GPU.OUR[ipver], arg=arg, out=outs, work=work, **kw)
        vfy(res["out"], res["out_off"][:k + 1], mask=mask, type=typ)

    # a first run outside capture (library and device-info setup), into outputs of its own
    chain(torch.empty_like(req), torch.empty_like(arg), None, torch.empty_like(mask), torch.empty_like(typ))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        chain(req, arg, outs, mask, typ)
    torch.cuda.synchronize()
    for x in (req, out, t["status"], mask):
        assert (host(x).view(np.uint8) == GPU.FILL).all()  # capture ran nothing
    for _ in range(2):
        g.replay()
        assert np.array_equal(host(req).view(np.uint32), wreq) and np.array_equal(host(arg).view(np.uint32), warg)
        got = {key: host(t[key]).view(GPU._DT[key]) for key in t}
        got["out"] = host(out)
        GPU.err_same(got, w, o, "graph replay")
        assert GPU.bits_of(mask, k).all()
        want_t = np.array([((int(wreq[f]) & 0xFF) << 8) | (int(wreq[f]) >> 8) for f in o["src_frame"]], np.uint16)
        assert np.array_equal(host(typ).view(np.uint16), want_t)
        for x in list(t.values()) + [out, req, arg, mask, typ]:
            x.view(torch.uint8).fill_(GPU.FILL)
        torch.cuda.synchronize()


@pytest.mark.parametrize("placement", [("straddle", 1), ("wrap_frame", 0)], ids=_far.pid)
@pytest.mark.parametrize("ipver", [4, 6])
def test_frames_past_two_to_the_32(arena, ipver, placement):  # noqa: F811
    """A batch whose offsets pass 2^32 (tests/_far.layout): one frame lies across byte 2^32 and every later one above
    it, or the span is 2^32 + len(f) bytes long and starts with a frame f that a kernel keeping only the low word of
    its length would answer. The span is BAD (no length field says 2^32), the far frames are answered exactly as the
    same frames of the compact twin, and nothing in 4 GiB is written."""
    rng = _rng(13, ipver, _far.PLACEMENTS.index(placement))
    near = [G.err_frame(rng, str(rng.choice(G.ERR_KINDS)), ipver, 100) for _ in range(100)]
    far = [G.err_frame(rng, str(rng.choice(G.ERR_KINDS, p=G._weights(len(G.ERR_KINDS)))), ipver, 1400) for _ in range(300)]
    f = _frame(rng, ipver, 120)
    head = f + rng.integers(0, 256, _far.HEAD - len(f), dtype=np.uint8).tobytes()
    if placement[0] == "wrap_frame":
        placement = ("wrap_frame", len(f))
    r = _far.layout(near, head, far, placement, lead=int(rng.integers(4)), rng=rng)
    req, arg = G.requests(rng, r.n, ipver, p_none=0.1)
    req[r.span] = 3
    GPU.put(arena, r.pieces())
    kw = dict(ident0=0x1234, max_out=r.n - 50)
    w, o = GPU.err_want(r.buf, r.offs, req, arg, ipver, **kw)
    assert o["status"][r.span] == M.BAD and (o["status"][r.span + 1:] == M.SENT).sum() > 60
    got = GPU.err_gpu(r.buf, r.offs, req, arg, ipver, d_buf=arena, d_offs=d(r.far_offs), dlead=3, **kw)
    GPU.err_same(got, w, o, "far offsets")
    GPU.check_arena(arena, r.pieces(), "err")
