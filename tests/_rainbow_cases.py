"""The fourteen synthetic rings of tests/_nstep_cases.py, imported as they are, each extended by Rainbow networks, a noise key and a support, with their float64
expectations — TEST INFRASTRUCTURE (tests/test_rainbow_cases_cpu.py validates it, tests/test_gpu_rainbow_cases.py uses it).  The reference is
tests/_rainbow_ref.py.

A case keeps its ring, indices, head, n_step, gamma and weights (every row kind placed, everything no walk reads NaN-poisoned: tests/_nstep_cases.py) and the TORSO of
its two dueling vectors, and adds
  heads     13,005 means U(+-1 / sqrt(84)) per network (x 30 on the ring scale_30_17: the softmax saturates and the 1e-8 decides logf)
  sigma     sigma_0 / sqrt(84) x U(0.5, 1.5) per element, an independent draw for the target network; times the family's scale (0, 1 or 8)
  the key   (noise_seed, u): the online sample is (u, 0), the target's (u, 1) on stream 14, from the float32 restatement; e_alt, the sample (u, 2), is the third
            sample of the conditions
  noisy     1, or 0 in the family "off"
  support   SUPPORT[name]: wide on most rings; the narrow (0, 4) on rings whose rewards are N(0, 1), so rows clamp at v_min and at v_max
Families are tests/_noisy_cases.py's, on the same rings.  The NOISY cases are those of default, sigma_x8, synced and weights_zero.

Placed distributional edges (EDGES[name] names what a ring must carry; `cond` counts them on the float64 reference):
  clamp_lo / clamp_hi   a row with an atom clamped at v_min / at v_max
  on_atom               a TERMINAL row (lg == 0) whose R lies exactly on an atom, l == u (through the clamp: R beyond the support)
  one_atom              a row whose whole target mass lands on one atom

Conditions, judged on the float64 reference (SEEDS holds the first seed from 0 that meets them; the seed moves heads, sigma and the key, never the ring).  No row is
excluded.  At EVERY bootstrap observation the online network's |q0 - q1| under the online sample is >= CLOSE_Q of the family; a* takes both values among the rows
whose last step did not terminate (more than one row); |loss| >= LOSS_FLOOR; the ring's EDGES are present.  A noisy case has a bootstrapping row whose argmax under
the third sample is not a*.
"""
import functools

import numpy as np

import _noisy_cases as NC
import _nstep_cases as K
import _rainbow_ref as Z

f32 = np.float32
LOSS_FLOOR = K.LOSS_FLOOR
NAMES, SPECS = K.NAMES, K.SPECS
FAMILY_OF, SCALE, NOISY_FAMILIES = NC.FAMILY_OF, NC.SCALE, NC.NOISY_FAMILIES
WIDE, NARROW = (-10.0, 10.0), (0.0, 4.0)
SUPPORT = dict(plain_1_n1=WIDE, plain_12_n2=NARROW, plain_13_n3=WIDE, plain_17_n5=NARROW, plain_129_n3=WIDE, plain_300_n16=NARROW, beyond_0_17=WIDE,
               weights_one_17=WIDE, weights_span_17=NARROW, synced_17=WIDE, gamma_0_17=NARROW, gamma_1_17=WIDE, scale_30_17=(-100.0, 100.0), kink_placed_17=WIDE)
_ALL = ("clamp_lo", "clamp_hi", "on_atom", "one_atom")
# what each narrow ring's fixed rewards and flags can carry (its terminal rows' R on both sides of the support or not)
EDGES = dict(plain_12_n2=("clamp_lo", "clamp_hi", "on_atom"), plain_17_n5=("clamp_lo", "clamp_hi"), plain_300_n16=_ALL, weights_span_17=_ALL,
             gamma_0_17=("clamp_lo", "on_atom", "one_atom"))
HEAD_SCALE = dict(scale_30_17=30.0)
# found by find_seed(i): the first seed from 0 whose case meets the conditions of the module docstring
SEEDS = (0, 0, 0, 3, 0, 0, 0, 1, 0, 1, 0, 0, 0, 1)


def build(i, seed):
    """case i from `seed`, with its float64 expectation under "exp" and the quantities the conditions are about under "cond" """
    base = K.make_case(i)
    name = base["name"]
    fam = FAMILY_OF[name]
    rng = np.random.default_rng([i, seed, 2018, 22])
    hs = HEAD_SCALE.get(name, 1.0)
    params = Z.vector(base["params"], rng, SCALE[fam], hs, jitter=True)
    target = Z.vector(base["target"], rng, SCALE[fam], hs, jitter=True)
    if base["family"] == "synced":
        target = params.copy()
    noise_seed, u = 2000 + 17 * i + seed, 3 + i
    e = lambda b: Z.eps(noise_seed, u, b, Z.STREAM_LEARN)   # noqa: E731
    c = dict(base, ring_family=base["family"], family=fam, params=params, target=target, noisy=0 if fam == "off" else 1, noise_seed=noise_seed, u=u,
             e_on=e(0), e_tg=e(1), e_alt=e(2), support=SUPPORT[name])
    del c["exp"], c["cond"]
    x = c["exp"] = Z.evaluate(c)
    live, boot, term = x["live"] > 0, x["lg"] != 0, x["lg"] == 0
    if c["noisy"]:
        obs = c["observations"].reshape(-1, 4)[x["at"]]
        alt = Z.forward(params, obs, c["support"], c["e_alt"])[1].argmax(axis=1)
    else:
        alt = x["next_actions"]
    tp = x["target_probs"]
    c["cond"] = dict(loss=x["loss"], q_gap=float(np.abs(x["q_next"][:, 0] - x["q_next"][:, 1]).min()), live=int(live.sum()), live_a1=int(x["next_actions"][live].sum()),
                     alt_flips=int((alt != x["next_actions"])[boot].sum()), clamp_lo=int(x["at_lo"].any(axis=1).sum()), clamp_hi=int(x["at_hi"].any(axis=1).sum()),
                     on_atom=int((x["same"].all(axis=1) & term).sum()), one_atom=int(((tp > 0).sum(axis=1) == 1).sum()))
    return c


def conditions_met(c):
    k = c["cond"]
    ok = abs(k["loss"]) >= LOSS_FLOOR and k["q_gap"] >= Z.CLOSE_Q[c["family"]]
    if c["mb"] > 1:
        ok = ok and 1 <= k["live_a1"] < k["live"]
    if c["family"] in NOISY_FAMILIES:
        ok = ok and k["alt_flips"] >= 1
    for edge in EDGES.get(c["name"], ()):
        ok = ok and k[edge] >= 1
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


def applies(variant, c):
    """whether the wrong reading `variant` must move case c"""
    x, k = c["exp"], c["cond"]
    boot = x["lg"] != 0
    if variant in ("no_noise", "target_shares_online_sample", "sigma_grad_unscaled"):
        return c["family"] in NOISY_FAMILIES
    if variant == "argmax_by_target_net":
        return bool((x["q_target"].argmax(axis=1) != x["next_actions"])[boot].any())
    if variant == "one_step_projection":
        return bool(((x["horizon"] > 1) & boot).any()) and c["gamma"] not in (0.0, 1.0)
    if variant == "projection_unclamped":
        return k["clamp_lo"] + k["clamp_hi"] > 0
    if variant == "l_equals_u_mass_dropped":
        return bool(x["same"].any())
    if variant in ("weights_ignored", "priority_weighted"):
        return c["weights"] is not None and bool((np.asarray(c["weights"]) != 1).any())
    if variant == "eps_inside_softmax_not_log":
        return c["name"] in HEAD_SCALE
    return True   # dueling_mean_missing
