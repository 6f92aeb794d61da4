"""Synthetic backbones with masked residues (test helper, imported like schedule_model.py; never imported by the product).

Two ways a residue ends up with mask 0 in alt_parse_PDB / tied_featurize, as in real training data:
  * its N line is missing: the residue keeps its letter, its N coordinates are NaN (make_golden.gapped_pdb, residue 120);
  * all four of its lines are missing: a numbering gap, filled with '-' (token 20, X) and NaN coordinates. A gap needs a residue on
    both sides; removing the first or last residue would only shorten the chain.
Indices here are 0-based residue positions; the PDB numbers residues from 1.
"""
import os

from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone

# name -> (L, backbone seed, residues without their N line, residues removed entirely). Each layout has a masked first residue,
# a masked last residue, isolated masked residues and a run of 3.
LAYOUTS = {
    # K = L: every row has masked neighbours (10 of 40 masked)
    "msk_L40": (40, 5, (0, 12, 30, 31, 39), (7, 20, 21, 22, 26)),
    # K = 48 < L with 46 unmasked residues: every unmasked row's top 48 holds masked neighbours at that row's D_max
    "msk_L56": (56, 5, (0, 9, 40, 41, 55), (18, 30, 31, 32, 47)),
}


def masked_pdb_text(L, seed, missing_n=(), gaps=()):
    """backbone_pdb_text of synthetic_backbone(L, seed) without the N line of ``missing_n`` and every line of ``gaps``."""
    assert all(0 < g < L - 1 for g in gaps), "a numbering gap needs residues on both sides"
    assert not set(missing_n) & set(gaps)
    X, seq = synthetic_backbone(L, seed)
    out = []
    for line in backbone_pdb_text(X, seq).split("\n"):
        if line.startswith("ATOM"):
            i = int(line[22:26]) - 1
            if i in gaps or (i in missing_n and line[12:16].strip() == "N"):
                continue
        out.append(line)
    return "\n".join(out)


def write_layout(name, directory):
    """Writes LAYOUTS[name] as <directory>/<name>.pdb -> its path."""
    L, seed, missing_n, gaps = LAYOUTS[name]
    path = os.path.join(str(directory), f"{name}.pdb")
    with open(path, "w") as fh:
        fh.write(masked_pdb_text(L, seed, missing_n, gaps))
    return path


def expected(name):
    """-> (mask as a list of 0 / 1, the positions that parse to '-') of LAYOUTS[name]."""
    L, _, missing_n, gaps = LAYOUTS[name]
    masked = set(missing_n) | set(gaps)
    return [0 if i in masked else 1 for i in range(L)], sorted(gaps)
