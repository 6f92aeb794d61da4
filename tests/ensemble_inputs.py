"""Crafted inputs for tmpnn_ensemble_stats, shared by tests/test_ensemble_host.py and tests/test_gpu_ensemble.py, which therefore see the
same tables, and the multi-MODEL file of the parser and end-to-end tests; no GPU, no torch. Two draws:
  "tie"       the pair-map POOL (+-0, +-inf, NaN, a denormal, 1 and 1 + ulp, a few small numbers): few values, so that sums and extremes
              tie and every special bit pattern takes part; ``plant_ties`` adds the cases a draw may miss.
  "rounding"  (standard normal x 1.5 - 0.3) as float32: sums and squared deviations that round, so that the ORDER of the sums and the
              separate rounding of the multiply decide bits.
S is drawn from [-2, 22): negative letters and 20, 21 take no part."""
import numpy as np

from test_pair_map_host import POOL

SHAPES = ((1, 19), (2, 70), (3, 19), (17, 70), (0, 5))     # (M, L) of the crafted batch: L = 70 x 20 letters = 1 400 entries, so the
                                                           # borders of the 256-entry tiles fall inside rows; M = 0 has output rows only
DRAWS = ("tie", "rounding")


def pack(shapes):
    """(M, L) per ensemble, contiguous and in order -> (desc [E, 4] int32, T, T_out, max_len)."""
    desc, row, out = [], 0, 0
    for M, L in shapes:
        desc.append((row, M, L, out))
        row, out = row + M * L, out + L
    return np.array(desc, np.int32).reshape(-1, 4), row, out, max([L for _, L in shapes], default=0)


def draw_table(draw, T, ld, rng):
    if draw == "tie":
        return POOL[rng.integers(0, len(POOL), size=(T, ld))]
    return (rng.standard_normal((T, ld)) * 1.5 - 0.3).astype(np.float32)


def plant_ties(ddg, S, desc):
    """Into the (3, 19) and (17, 70) ensembles of a tie draw, in place, what the draw may miss. At position q of each:
      q = 4   every member out (S = 20, -1, 21, ...): count 0 in all 20 letters
      q = 5   letter 3: NaN in every member, the members themselves in: a NaN-only entry
      q = 6   letter 7: +inf at member 0, -inf at member 1: a NaN mean and spread beside lo = -inf, hi = +inf
      q = 7   letter 2: 1, -0.0, +0.0, 1 ...: lo is the -0.0 of member 1 (its own bits), not the +0.0 of member 2
      q = 8   letter 2: -1, +0.0, -0.0, -1 ...: hi is the +0.0 of member 1
      q = 9   letter 2: -0.0, +0.0, 1, 1 ...: lo is member 0's -0.0
    -> [(ensemble, q)] of the planted positions."""
    bits = ddg.view(np.uint32)
    sites = []
    for e in (2, 3):
        row0, M, L, _ = (int(v) for v in desc[e])
        rows = lambda q: row0 + np.arange(M) * L + q
        S[rows(4)] = np.array([20, -1, 21, -2] * M)[:M]
        for q in (5, 6, 7, 8, 9):
            S[rows(q)] = 11
        bits[rows(5), 3] = 0x7fc00000
        bits[rows(6)[2:], 7] = 0x3f800000
        bits[rows(6)[0], 7], bits[rows(6)[1], 7] = 0x7f800000, 0xff800000
        ddg[rows(7), 2] = 1.0
        bits[rows(7)[1], 2], bits[rows(7)[2], 2] = 0x80000000, 0
        ddg[rows(8), 2] = -1.0
        bits[rows(8)[1], 2], bits[rows(8)[2], 2] = 0, 0x80000000
        ddg[rows(9), 2] = 1.0
        bits[rows(9)[0], 2], bits[rows(9)[1], 2] = 0x80000000, 0
        sites += [(e, q) for q in range(4, 10)]
    return sites


def crafted(draw, seed=7, ld=21, shapes=SHAPES):
    """dict(ddg [T, ld], S [T], desc, T, T_out, max_len, members, lengths) for one batch of ``shapes``."""
    rng = np.random.default_rng(seed + (0 if draw == "tie" else 100))
    desc, T, T_out, max_len = pack(shapes)
    ddg = draw_table(draw, T, ld, rng)
    S = rng.integers(-2, 22, size=T).astype(np.int32)
    c = dict(ddg=ddg, S=S, desc=desc, T=T, T_out=T_out, max_len=max_len, members=[M for M, _ in shapes], lengths=[L for _, L in shapes])
    if draw == "tie" and shapes == SHAPES:
        c["sites"] = plant_ties(ddg, S, desc)
    return c


def single(draw, M, L, seed):
    """One ensemble of M members of L rows, every row in (S in [0, 20)) — the conditions on the order of the sums are counted on it."""
    rng = np.random.default_rng(seed)
    c = crafted(draw, seed, shapes=((M, L),))
    c["S"] = rng.integers(0, 20, size=c["T"]).astype(np.int32)
    return c


def ulp_cutoff(c):
    """A cutoff one ulp BELOW a table value that takes part (so x <= cutoff is false for that value and true one ulp on), and the
    value: the middle entry, by value, of the participating finite entries of letter 0."""
    ok = (c["S"] >= 0) & (c["S"] < 20) & np.isfinite(c["ddg"][:, 0])
    v = np.sort(c["ddg"][ok, 0])[ok.sum() // 2]
    return float(np.nextafter(np.float32(v), np.float32(-np.inf))), float(v)


# ---- structures --------------------------------------------------------------------------------------------------------------------
def write_models(path, L=40, seed=3, n=3, drop=None):
    """A multi-MODEL file: ``n`` jittered conformers of synthetic_backbone(L, seed), coordinates rounded to three decimals (what the
    file holds). ``drop`` = (model, residue): that model's N line of that residue is left out. -> (X [n, L, 4, 3], seq)."""
    from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone
    X0, seq = synthetic_backbone(L, seed)
    rng = np.random.default_rng(seed + 50)
    X = np.round(X0[None] + rng.normal(0.0, 0.25, size=(n,) + X0.shape), 3)
    text = []
    for m in range(n):
        lines = backbone_pdb_text(X[m], seq).split("\n")
        lines = [ln for ln in lines if ln.startswith("ATOM")]
        if drop is not None and drop[0] == m:
            lines = [ln for ln in lines if not (ln[12:16] == " N  " and int(ln[22:26]) == drop[1] + 1)]
        text += [f"MODEL     {m + 1:4d}"] + lines + ["TER", "ENDMDL"]
    with open(path, "w") as fh:
        fh.write("\n".join(text + ["END", ""]))
    return X, seq
