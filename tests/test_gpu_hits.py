"""Ranked hit lists on the device (tmpnn_select_hits, Engine.select_hits, TransferModel.hit_list, scan_to_file(top=k)) against the
numpy restatement of the contract (tests/hits_restatement.py). Every comparison is exact: value bits, positions, letters, counts."""
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, weights_for_case
from hits_restatement import assert_hits_equal, hits_reference

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
POOL = np.array([-3.0, -1.5, -0.0, 0.0, 0.25, NAN, INF, -INF], np.float32)     # eight values: ties dominate
B = 256                                                                        # residues per stage-1 block (csrc/tmpnn_hits.hip)


@pytest.fixture(scope="module")
def engine(synthetic_weights):
    from thermompnn_amd.engine import Engine
    return Engine(synthetic_weights, "cuda:0", 48)


def _crafted(lengths, seed, ld=21):
    """A table drawn from POOL and letters drawn from 0..20 (20 = no residue) for a ragged batch."""
    rng = np.random.default_rng(seed)
    T = int(sum(lengths))
    table = POOL[rng.integers(0, len(POOL), size=(T, ld))]
    S = rng.integers(0, 21, size=T).astype(np.int32)
    return table, S, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


@pytest.fixture(scope="module")
def ragged():
    """P = 37: every length at which the launch shape changes (1, 2, B - 1, B, B + 1, 2 B + 1), six times over, and one more protein
    without a single residue letter. Protein 3 is all cysteine wild types, protein 5 has S = 20 everywhere."""
    lengths = [1, 2, B - 1, B, B + 1, 2 * B + 1] * 6 + [B + 1]
    table, S, offsets = _crafted(lengths, 7)
    S[0] = 4                                                 # protein 0: one residue with a letter
    S[offsets[3]:offsets[4]] = 1
    S[offsets[5]:offsets[6]] = 20
    S[offsets[36]:offsets[37]] = 20
    assert len(lengths) == 37
    return table, S, offsets


def _run(engine, table, S, offsets, k, **kw):
    return engine.select_hits(torch.from_numpy(table).cuda(), S, offsets, k, **kw)


def test_ragged_batch_with_ties_every_k_flag_and_cutoff(engine, ragged):
    table, S, offsets = ragged
    dev = torch.from_numpy(table).cuda()
    for k in (1, 7, 256):
        for cys in (False, True):
            for one in (False, True):
                for cutoff in (None, 0.0):
                    got = engine.select_hits(dev, S, offsets, k, cutoff=cutoff, include_cys=cys, one_per_position=one)
                    want = hits_reference(table, S, offsets, k, cutoff, cys, one)
                    assert_hits_equal(got, want)
    full = {k_: v.cpu().numpy() for k_, v in engine.select_hits(dev, S, offsets, 256).items()}
    assert full["hit_count"][5] == 0 and full["hit_count"][36] == 0 and np.isnan(full["hit_ddg"][5]).all() and (full["hit_pos"][5] == -1).all()
    assert not (full["hit_aa"][3] == 1).any() and full["hit_count"][3] == 256        # wild type C, no include_cys: C never appears
    assert full["hit_count"].max() == 256 and 0 < full["hit_count"][0] < 20           # one residue: fewer candidates than k
    # a cutoff below every value: no candidate anywhere (the table without its -inf entries, so that such a cutoff exists)
    finite_low = np.where(np.isneginf(table), np.float32(-3.0), table)
    got = _run(engine, finite_low, S, offsets, 7, cutoff=-1e30)
    assert_hits_equal(got, hits_reference(finite_low, S, offsets, 7, -1e30))
    assert int(got["hit_count"].sum()) == 0 and bool(torch.isnan(got["hit_ddg"]).all())
    # a cutoff of -inf keeps exactly the -inf entries; a row stride above 21 is the table's leading dimension
    assert_hits_equal(engine.select_hits(dev, S, offsets, 7, cutoff=-INF), hits_reference(table, S, offsets, 7, -INF))
    wide = torch.full((table.shape[0], 24), 5.0, device="cuda")
    wide[:, :21] = dev
    assert_hits_equal(engine.select_hits(wide[:, :21], S, offsets, 7), hits_reference(table, S, offsets, 7))


@pytest.mark.parametrize("one", [False, True])
def test_one_protein_of_8192_residues_runs_the_full_merge(engine, one):
    table, S, offsets = _crafted([8192], 3)
    got = _run(engine, table, S, offsets, 256, one_per_position=one)
    assert_hits_equal(got, hits_reference(table, S, offsets, 256, one_per_position=one))
    # distinct values in descending order of position: the hits come from the LAST block, through all 32 leaders' merge
    table2 = np.full((8192, 21), NAN, np.float32)
    table2[:, 5] = -np.arange(8192, dtype=np.float32)
    S2 = np.zeros(8192, np.int32)
    got2 = _run(engine, table2, S2, offsets, 256, one_per_position=one)
    assert_hits_equal(got2, hits_reference(table2, S2, offsets, 256, one_per_position=one))
    assert got2["hit_pos"][0, :3].tolist() == [8191, 8190, 8189]
    from thermompnn_amd._lib import TmpnnError
    with pytest.raises(TmpnnError, match="8192"):
        _run(engine, np.zeros((8193, 21), np.float32), np.zeros(8193, np.int32), [0, 8193], 4)


def test_a_protein_alone_equals_itself_in_the_batch_and_reruns_give_equal_bits(engine, ragged):
    table, S, offsets = ragged
    dev = torch.from_numpy(table).cuda()
    for kw in (dict(), dict(one_per_position=True, include_cys=True, cutoff=0.25)):
        a = {k_: v.cpu().numpy() for k_, v in engine.select_hits(dev, S, offsets, 7, **kw).items()}
        b = {k_: v.cpu().numpy() for k_, v in engine.select_hits(dev, S, offsets, 7, **kw).items()}
        for name in a:
            np.testing.assert_array_equal(a[name].view(np.uint32) if a[name].dtype == np.float32 else a[name],
                                          b[name].view(np.uint32) if b[name].dtype == np.float32 else b[name])
        for p in (0, 2, 4, 5, 11, 36):                      # lengths 1, B - 1, B + 1, 2 B + 1 (no letters), 2 B + 1, the last protein
            t0, t1 = int(offsets[p]), int(offsets[p + 1])
            alone = engine.select_hits(dev[t0:t1], S[t0:t1], [0, t1 - t0], 7, **kw)
            assert_hits_equal(alone, {name: v[p:p + 1] for name, v in a.items()})


def _fixture_entry(g, name):
    """A parsed-structure dict (the shape alt_parse_PDB produces) holding a fixture's own coordinates and sequence."""
    from thermompnn_amd.datasets import ALPHABET
    seq = "".join(ALPHABET[int(s)] for s in g["S"])
    coords = {f"{a}_chain_A": g["X"][:, i].astype(np.float64).tolist() for i, a in enumerate(("N", "CA", "C", "O"))}
    return {"resn_list": [str(i + 1) for i in range(len(seq))], "seq_chain_A": seq, "coords_chain_A": coords, "name": name,
            "num_of_chains": 1, "seq": seq}


@pytest.mark.parametrize("case", ["syn_L32", "2OCJ_A"])
def test_hits_of_the_fused_forward_and_hit_list(case):
    from thermompnn_amd import custom_inference
    from thermompnn_amd.datasets import ALPHABET
    from thermompnn_amd.engine import Engine
    from thermompnn_amd.pdb_io import alt_parse_PDB
    g = load_golden(case)
    eng = Engine(weights_for_case(g), "cuda:0", 48)
    L = g["X"].shape[0]
    S, offsets = g["S"].astype(np.int32), np.array([0, L], np.int32)
    ddg = eng.ssm_forward(g["X"], S, g["mask"], g["residue_idx"], g["chain_enc"], offsets)["ddg"]        # stays on the device
    back = ddg.cpu().numpy()
    for kw in (dict(), dict(one_per_position=True), dict(cutoff=float(np.median(back[:, :20])), include_cys=True)):
        assert_hits_equal(eng.select_hits(ddg, S, offsets, 32, **kw), hits_reference(back, S, offsets, 32, kw.get("cutoff"),
                                                                                    kw.get("include_cys", False), kw.get("one_per_position", False)))
    # TransferModel.hit_list: one forward, one selection, Mutation objects best first
    model = custom_inference.load_model(None, None, int(g["weight_seed"]))
    pdb = alt_parse_PDB(os.path.join(GOLDEN, "2OCJ.pdb"), "A") if case == "2OCJ_A" else [_fixture_entry(g, case)]
    seq = pdb[0]["seq"]
    with torch.no_grad():
        table = model.ssm_table(pdb).cpu().numpy()
        for kw in (dict(), dict(one_per_position=True, cutoff=0.0)):
            hits = model.hit_list(pdb, 12, **kw)
            Sq = np.array([ALPHABET.index(c) if c in ALPHABET[:20] else 20 for c in seq], np.int32)
            want = hits_reference(table, Sq, [0, len(seq)], 12, kw.get("cutoff"), False, kw.get("one_per_position", False))
            n = int(want["hit_count"][0])
            assert n > 0 and len(hits) == n
            assert [(m.position, m.mutation) for m in hits] == [(int(p), ALPHABET[int(a)]) for p, a in zip(want["hit_pos"][0, :n], want["hit_aa"][0, :n])]
            assert [m.wildtype for m in hits] == [seq[m.position] for m in hits] and all(m.pdb == pdb[0]["name"] for m in hits)
            np.testing.assert_array_equal(np.array([m.ddG for m in hits], np.float32).view(np.uint32), want["hit_ddg"][0, :n].view(np.uint32))
            assert [m.ddG for m in hits] == sorted(m.ddG for m in hits)


def _pdb_set(tmp_path, n=23, seed=11):
    """The file set of tests/test_gpu_e2e.py: synthetic backbones of 20..199 residues, 2OCJ, and 2OCJ with numbering gaps."""
    from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone
    rng = np.random.default_rng(seed)
    paths = []
    for i, L in enumerate(rng.integers(20, 200, size=n)):
        X, seq = synthetic_backbone(int(L), 9000 + i)
        p = tmp_path / f"syn_{i:03d}.pdb"
        p.write_text(backbone_pdb_text(X, seq))
        paths.append(str(p))
    paths.insert(3, os.path.join(GOLDEN, "2OCJ.pdb"))
    paths.insert(9, os.path.join(GOLDEN, "2OCJ_gap_chainA.pdb"))
    return paths


def _csv_from_npz(npz_path, out, k, **kw):
    from thermompnn_amd import ssm_scan
    z = np.load(npz_path)
    seqs, names = [str(s) for s in z["seqs"]], [str(n) for n in z["names"]]
    want = hits_reference(z["ddg"], ssm_scan.sequence_letters(seqs), z["offsets"], k, kw.get("cutoff"), kw.get("include_cys", False),
                          kw.get("one_per_position", False))
    ssm_scan.write_hits_csv(out, want, seqs, names)
    return want


def test_scan_to_hit_csv_equals_the_restatement_on_the_binary_scan_and_the_cli(tmp_path, engine):
    from thermompnn_amd import ssm_scan
    paths = _pdb_set(tmp_path)
    ch = ["A"] * len(paths)
    ssm_scan.scan_to_file(engine, paths, ch, str(tmp_path / "scan.npz"), chunk_files=7, chunk_residues=600)
    want = _csv_from_npz(tmp_path / "scan.npz", str(tmp_path / "want.csv"), 5)
    n, stats = ssm_scan.scan_to_file(engine, paths, ch, str(tmp_path / "hits.csv"), top=5, chunk_files=7, chunk_residues=600, parse_threads=3)
    assert n == int(want["hit_count"].sum()) == 5 * len(paths) and stats.files == len(paths) and stats.chunks >= 4 and stats.reruns == 0
    got = (tmp_path / "hits.csv").read_bytes()
    assert got == (tmp_path / "want.csv").read_bytes()
    assert got.startswith(b",Model,Dataset,ddG_pred,position,wildtype,mutation,rank,pdb\n0,ThermoMPNN,custom,")
    # the other options reach the selection
    kw = dict(cutoff=-0.5, include_cys=True, one_per_position=True)
    _csv_from_npz(tmp_path / "scan.npz", str(tmp_path / "want2.csv"), 40, **kw)
    ssm_scan.scan_to_file(engine, paths, ch, str(tmp_path / "hits2.csv"), top=40, chunk_files=7, chunk_residues=600, **kw)
    assert (tmp_path / "hits2.csv").read_bytes() == (tmp_path / "want2.csv").read_bytes()
    # the CLI equals the library call byte for byte
    cli = ssm_scan.main(paths + ["--synthetic_weights", "0", "--out", str(tmp_path / "cli.csv"), "--chunk_files", "3", "--top", "40",
                                 "--cutoff", "-0.5", "--include_cys", "--one_per_position"])
    assert open(cli, "rb").read() == (tmp_path / "hits2.csv").read_bytes()
    assert ssm_scan.scan_to_file(engine, [], [], str(tmp_path / "empty.csv"), top=5)[0] == 0
    assert (tmp_path / "empty.csv").read_bytes() == b",Model,Dataset,ddG_pred,position,wildtype,mutation,rank,pdb\n"


def test_hits_of_a_rerun_chunk_come_from_the_rerun_table(tmp_path, synthetic_weights):
    """The edge-embedding x 1e6 weights of test_pipeline_reruns_an_overflowing_chunk: every f16x2 chunk leaves the fp16 range and is
    rerun in bf16x3 into the same rows of the device table; the hit list is selected afterwards, so it equals a bf16x3 engine's."""
    from thermompnn_amd import ssm_scan
    from thermompnn_amd.engine import Engine
    W = {k: v.clone() for k, v in synthetic_weights.items()}
    W["prot_mpnn.features.edge_embedding.weight"] = W["prot_mpnn.features.edge_embedding.weight"] * 1e6
    paths = _pdb_set(tmp_path, n=6, seed=3)
    ch = ["A"] * len(paths)
    ssm_scan.scan_to_file(Engine(W, "cuda:0", 48, precision="bf16x3"), paths, ch, str(tmp_path / "want.csv"), top=9, chunk_files=3)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        _, stats = ssm_scan.scan_to_file(Engine(W, "cuda:0", 48, precision="f16x2"), paths, ch, str(tmp_path / "got.csv"), top=9, chunk_files=3)
    assert stats.reruns == stats.chunks >= 2 and any("bf16x3" in str(w.message) for w in rec)
    got = (tmp_path / "got.csv").read_bytes()
    assert got == (tmp_path / "want.csv").read_bytes() and got.count(b"\n") == 1 + 9 * len(paths) and b"nan" not in got


def test_native_host_example_writes_the_same_hit_list(tmp_path, engine, synthetic_weights):
    """examples/scan_native.cpp --top K: a host without Python reaches the selection through the C-ABI alone (the table of
    tmpnn_ssm_forward stays in its device buffer) and writes the bytes of the Python scan, also over several chunks and with every
    option."""
    import subprocess
    from thermompnn_amd import build, ssm_scan, weights
    exe = os.path.join(os.path.dirname(build.HERE), "examples", "scan_native")
    if not os.path.exists(exe):
        build.build_native_example()
    raw = str(tmp_path / "w.raw")
    weights.export_raw(synthetic_weights, raw)
    paths = _pdb_set(tmp_path, n=9, seed=3)
    for k, extra, kw in ((5, [], {}), (40, ["--chunk_files", "4", "--cutoff", "-0.5", "--one_per_position", "--include_cys"],
                                      dict(cutoff=-0.5, one_per_position=True, include_cys=True))):
        ref, out = str(tmp_path / "py.csv"), str(tmp_path / "native.csv")
        n, _ = ssm_scan.scan_to_file(engine, paths, ["A"] * len(paths), ref, top=k, **kw)
        r = subprocess.run([exe, raw, out, "--top", str(k)] + extra + paths, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.startswith(f"{n} rows, ") and n > 0
        assert open(out, "rb").read() == open(ref, "rb").read()
    r = subprocess.run([exe, raw, str(tmp_path / "x.csv"), "--top", "300"] + paths[:1], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "--top" in r.stderr
