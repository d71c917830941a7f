"""Seeded random batches through the three ICMP passes on the GPU (tests/_icmp_gen.py: 20 seeds per pass and IP version,
each with random launch overrides of nsx_icmp_tune.h), every output array and every untouched region bit-exact against
tests/_icmp.py. tests/test_icmp_gen.py shows on any host that no seed is vacuous."""
import numpy as np
import pytest

import _icmp_gen as G
import _icmp_gpu as GPU
from _gpu import setup_gpu

pytestmark = pytest.mark.gpu


def setup_module(module):
    setup_gpu()


def _tune(kind, ipver, seed):
    return G.tune(np.random.default_rng([0x1C3F, 9, kind, ipver, seed]))


@pytest.mark.parametrize("seed", range(G.SEEDS))
@pytest.mark.parametrize("ipver", [4, 6])
def test_error_generation(ipver, seed):
    buf, offs, req, arg, kw = G.err_batch(seed, ipver)
    tune = _tune(1, ipver, seed)
    GPU.err_check(buf, offs, req, arg, ipver, tunes=(tune,), dleads=(seed % 16,), what=f"seed {seed}", **kw)


@pytest.mark.parametrize("seed", range(G.SEEDS))
@pytest.mark.parametrize("ipver", [4, 6])
def test_receive_verify(ipver, seed):
    buf, offs, _ = G.rx_batch(seed, ipver)
    GPU.rx_check(buf, offs, ipver, tunes=(_tune(2, ipver, seed),), what=f"seed {seed}")


@pytest.mark.parametrize("seed", range(G.SEEDS))
@pytest.mark.parametrize("ipver", [4, 6])
def test_echo_reply(ipver, seed):
    buf, offs, valid, ttl = G.echo_batch(seed, ipver)
    GPU.echo_check(buf, offs, valid, ttl, ipver, what=f"seed {seed}")
