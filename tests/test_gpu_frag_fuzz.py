"""Fragmentation and reassembly fuzzed on the GPU: 20 seeded batches per pass from tests/_frag_gen.py, each under random
launch overrides, compared bit for bit with the numpy restatement tests/_frag.py (tests/test_frag_gen.py shows that no
seed is vacuous)."""
import numpy as np
import pytest

import _frag_gen as GEN
import _frag_gpu as GPU
from _gpu import setup_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    setup_gpu()


@pytest.mark.parametrize("seed", GEN.SEEDS)
def test_frag_fuzz(seed):
    rng = np.random.default_rng([0xF6C2, seed])
    buf, offs, mtu = GEN.frag_batch(seed)
    GPU.frag_check(buf, offs, mtu, (GEN.tune(rng), GEN.tune(rng)), dleads=(int(rng.integers(16)),), what=f"seed={seed}")


@pytest.mark.parametrize("seed", GEN.SEEDS)
def test_reasm_fuzz(seed):
    rng = np.random.default_rng([0xF6C3, seed])
    buf, offs = GEN.reasm_batch(seed)
    GPU.reasm_check(buf, offs, (GEN.tune(rng), GEN.tune(rng)), what=f"seed={seed}")
