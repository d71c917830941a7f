"""No seed of the ICMP fuzz (tests/test_gpu_icmp_fuzz.py over tests/_icmp_gen.py) is vacuous — a condition on the
generator, checked on any host with the model tests/_icmp.py: every error batch holds all five statuses, every verify
batch a valid frame and an invalid frame of each kind, every echo batch an answered and an unanswered request."""
import numpy as np
import pytest

import _icmp as M
import _icmp_gen as G


@pytest.mark.parametrize("ipver", [4, 6])
def test_every_error_batch_holds_all_five_statuses(ipver):
    for seed in range(G.SEEDS):
        buf, offs, req, arg, kw = G.err_batch(seed, ipver)
        r = M.err(buf, offs, req, arg, ipver=ipver, **kw)
        cnt = np.bincount(r["status"], minlength=5)
        assert (cnt >= 5).all(), (seed, cnt)
        assert r["n_out"] == kw["max_out"] == cnt[M.SENT] and cnt[M.LIMITED] >= 1
        lens = np.diff(r["out_off"])
        assert lens.max() == M.HDR[ipver] + M.QUOTE[ipver] and (lens % 2).any() and not (lens % 2).all(), seed


@pytest.mark.parametrize("ipver", [4, 6])
def test_every_verify_batch_holds_a_valid_and_an_invalid_frame_of_each_kind(ipver):
    for seed in range(G.SEEDS):
        buf, offs, kinds = G.rx_batch(seed, ipver)
        ok = M.verify(buf, offs, ipver)["ok"]
        kinds = np.array(kinds)
        assert set(kinds) == set(G.RX_KINDS[ipver])
        for k in G.RX_KINDS[ipver]:
            at = kinds == k
            assert at.sum() >= 2 and (ok[at].all() if k == "valid" else not ok[at].any()), (seed, k)
        lens = np.diff(offs)
        assert lens.max() > 296 and (ok & (lens > 296)).any() and (ok & (lens <= 296)).any(), seed  # both sum paths


@pytest.mark.parametrize("ipver", [4, 6])
def test_every_echo_batch_holds_an_answered_and_an_unanswered_request(ipver):
    rq = 8 if ipver == 4 else 128
    for seed in range(G.SEEDS):
        buf, offs, valid, ttl = G.echo_batch(seed, ipver)
        out, hit = M.echo(buf, offs, valid, ttl, ipver)
        fr = M.frames_of(buf, offs)
        is_rq = np.array([M.wellformed(f, ipver) is not None and f[M.wellformed(f, ipver)] == rq for f in fr])
        ok = M.verify(buf, offs, ipver)["ok"]
        assert (hit & is_rq).sum() >= 50 and (~hit & is_rq & valid).sum() >= 5 and (~hit & is_rq & ~valid).sum() >= 5, seed
        assert (hit & ~ok).sum() >= 3, seed  # a wrong checksum under a set bit is answered, and stays wrong
        assert not hit[~is_rq].any() and not np.array_equal(out, buf)
