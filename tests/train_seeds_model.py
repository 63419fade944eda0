"""CPU model of the device-side seed table of a captured training iteration (paella_amd/csrc/train_seeds.hip, paella_amd.training.TrainSeeds), written over the
Philox model of tests/counter_noise.py and independent of paella_amd.

The contract it states: the table is (base, iteration, word[0 .. n)); one advance sets iteration += 1 and then, for every site s,
    word[s] = w0 | w1 << 32,   (w0, w1, w2, w3) = philox4x32(key = base, counter (ctr_lo = s, ctr_hi = iteration))
so a word is a function of (base, iteration, site) alone -- not of n, and not of the words before it.  word[s] is the 64-bit seed the dropout op at drawing site s
of the forward takes: its mask is that of a by-value call with seed = word[s] (tests/grn_act_model.py, tests/attn_train_model.py)."""
import numpy as np

from tests import counter_noise as CN


def word(base, iteration, site):
    """one word, by the plain-integer transcription of Philox"""
    w = CN.philox4x32_scalar(int(base) & CN.M64, int(site), int(iteration) & CN.M64)
    return w[0] | (w[1] << 32)


def words(base, iteration, n_sites):
    """the n_sites words of one iteration as Python ints, vectorised"""
    w0, w1, _, _ = CN.philox4x32(int(base) & CN.M64, np.arange(n_sites, dtype=np.uint64), int(iteration) & CN.M64)
    return [int(a) | (int(b) << 32) for a, b in zip(w0, w1)]


class Table:
    """the table as the device holds it: `advance()` as the kernel, `values()` as TrainSeeds.values()"""

    def __init__(self, n_sites, base):
        self.n_sites, self.base, self.iteration = n_sites, int(base) & CN.M64, 0
        self.word = [0] * n_sites

    def advance(self):
        self.iteration = (self.iteration + 1) & CN.M64
        self.word = words(self.base, self.iteration, self.n_sites)
        return self

    def values(self):
        return list(self.word)
