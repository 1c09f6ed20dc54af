"""The fourteen synthetic rings of tests/_nstep_cases.py, imported as they are, each extended by a sigma vector and a noise key, with their float64 expectations —
TEST INFRASTRUCTURE (tests/test_noisy_cases_cpu.py validates it, tests/test_gpu_noisy_cases.py uses it).  The reference is tests/_noisy_ref.py.

A case keeps its ring, indices, head, n_step, gamma, weights and the two 11,019-float dueling vectors (every row kind placed, everything no walk reads poisoned:
tests/_nstep_cases.py) and adds
  sigma     255 floats behind each vector: sigma_0 / sqrt(84) x U(0.5, 1.5) per element (a constant would hide a permuted index), an independent draw for the target
            network; times `scale` (0, 1 or 8)
  the key   (noise_seed, u): the online sample is (u, 0), the target's (u, 1) on stream 14 under noise_seed, xi from the float32 restatement; xi_alt, the sample
            (u, 2), is what the wrong reading fresh_sample_for_argmax gives the argmax
  noisy     1, or 0 in the family "off"
Families (FAMILY_OF: which ring carries which):
  sigma_0       sigma == 0 with noisy = 1: the draw is made, the values are the mean network's, the sigma gradient is g * eps
  default       plain rings of every shape — one row, 12, 13, 17, 129 and 300 rows, n_step 1 .. 16 — and the placed exact-zero pre-activations
  sigma_x8      sigma x 8: the noise dominates the means
  off           noisy = 0 with non-zero sigma: the anchor (gamma 0 and weights of exactly 1 ride here)
  synced        target == online parameters bit for bit, sigma included: the two samples must still differ
  weights_zero  spanning weights with one exact 0
The NOISY cases — those a wrong reading of the noise must move — are the cases of default, sigma_x8, synced and weights_zero.

Conditions, judged on the float64 reference (SEEDS holds the first seed from 0 that meets them, find_seed; the seed moves sigma and the key, never the ring).  No
row is excluded from any comparison.  At EVERY bootstrap observation the online network's |q0 - q1| under the online sample is >= CLOSE_Q of the family; a* takes
both values among the rows that bootstrap (more than one row); |loss| >= LOSS_FLOOR.  A noisy case moreover has a bootstrapping row whose argmax under xi_alt is
not a*: without one no update could tell which sample chose the action.
"""
import functools

import numpy as np

import _noisy_ref as Z
import _nstep_cases as K

f32 = np.float32
LOSS_FLOOR = K.LOSS_FLOOR
NAMES, SPECS = K.NAMES, K.SPECS
FAMILY_OF = dict(plain_1_n1="default", plain_12_n2="default", plain_13_n3="sigma_x8", plain_17_n5="default", plain_129_n3="default", plain_300_n16="default",
                 beyond_0_17="sigma_0", weights_one_17="off", weights_span_17="weights_zero", synced_17="synced", gamma_0_17="off", gamma_1_17="sigma_x8",
                 scale_30_17="sigma_0", kink_placed_17="default")
SCALE = dict(sigma_0=0.0, default=1.0, sigma_x8=8.0, off=1.0, synced=1.0, weights_zero=1.0)
NOISY_FAMILIES = ("default", "sigma_x8", "synced", "weights_zero")
# found by find_seed(i): the first seed from 0 whose case meets the conditions of the module docstring
SEEDS = (1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 6, 0, 0)


def build(i, seed):
    """case i from `seed`, with its float64 expectation under "exp" and the quantities the conditions are about under "cond" """
    base = K.make_case(i)
    fam = FAMILY_OF[base["name"]]
    rng = np.random.default_rng([i, seed, 2018, 21])
    sig = lambda: (Z.default_sigma(SCALE[fam]) * rng.uniform(0.5, 1.5, Z.NHEAD).astype(f32)).astype(f32)   # noqa: E731
    params = np.concatenate([base["params"].astype(f32), sig()])
    target = np.concatenate([base["target"].astype(f32), sig()])
    if base["family"] == "synced":
        target = params.copy()
    noise_seed, u = 1000 + 17 * i + seed, 3 + i
    c = dict(base, ring_family=base["family"], family=fam, params=params, target=target, noisy=0 if fam == "off" else 1, noise_seed=noise_seed, u=u,
             xi_on=Z.xi(noise_seed, u, 0, Z.STREAM_LEARN), xi_tg=Z.xi(noise_seed, u, 1, Z.STREAM_LEARN), xi_alt=Z.xi(noise_seed, u, 2, Z.STREAM_LEARN))
    del c["exp"], c["cond"]
    e = c["exp"] = Z.evaluate(c)
    live, boot = e["live"] > 0, e["lg"] != 0   # (as tests/_nstep_cases.py counts a*: the rows whose last step did not terminate; boot: those whose target has a bootstrap term)
    alt = Z.evaluate(c, variant="fresh_sample_for_argmax")["next_actions"] if c["noisy"] else e["next_actions"]
    c["cond"] = dict(loss=e["loss"], q_gap=float(np.abs(e["q_next"][:, 0] - e["q_next"][:, 1]).min()), live=int(live.sum()), live_a1=int(e["next_actions"][live].sum()),
                     alt_flips=int((alt != e["next_actions"])[boot].sum()))
    return c


def conditions_met(c):
    k = c["cond"]
    ok = abs(k["loss"]) >= LOSS_FLOOR and k["q_gap"] >= Z.CLOSE_Q[c["family"]]
    if c["mb"] > 1:
        ok = ok and 1 <= k["live_a1"] < k["live"]
    if c["family"] in NOISY_FAMILIES:
        ok = ok and k["alt_flips"] >= 1
    return bool(ok)


def find_seed(i, start=0, tries=400):
    for seed in range(start, start + tries):
        if conditions_met(build(i, seed)):
            return seed
    raise RuntimeError("no seed for case %d" % i)


@functools.lru_cache(maxsize=None)
def make_case(i):
    """case i (cached: treat as read-only)"""
    return build(i, SEEDS[i])


def noisy_cases():
    return [i for i in range(len(SPECS)) if FAMILY_OF[NAMES[i]] in NOISY_FAMILIES]
