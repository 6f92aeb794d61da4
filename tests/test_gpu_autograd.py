"""TransferModel through torch autograd on the MI355X: the reference golden through loss.backward(), the split C-ABI against the fused
step bit for bit, arbitrary upstream gradients, the frozen encoder, gradient accumulation, a torch optimiser loop against MPNNTrainer,
and the default (non-differentiable) path left as it was."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, REPO, load_golden
from test_gpu_finetune import AA20, CASES, NF0, RELEASED, _case_mutants, _golden_sample_index, _mutants, _pdb, restate
from train_weight_cases import UPSTREAM_CASE

pytestmark = pytest.mark.gpu


def _cfg(tmp_path, head=None, subtract=True, freeze=False, training=None):
    from thermompnn_amd.train import Config
    head = head or RELEASED
    d = dict(model=dict(hidden_dims=list(head["hidden_dims"]), subtract_mut=subtract, num_final_layers=head["num_final_layers"],
                        freeze_weights=freeze, load_pretrained=True, lightattn=head["lightattn"]),
             platform=dict(thermompnn_dir=str(tmp_path)))
    if training:
        d["training"] = training
    return Config.wrap(d)


def _model(tmp_path, head=None, subtract=True, freeze=False, seed=0, style="xavier"):
    from thermompnn_amd import weights
    from thermompnn_amd.transfer_model import TransferModel
    head = head or RELEASED
    sd = weights.synthetic_state_dict(seed, style=style, head=head)
    vdir = os.path.join(str(tmp_path), "vanilla_model_weights")
    os.makedirs(vdir, exist_ok=True)
    weights.save_vanilla_checkpoint(os.path.join(vdir, "v_48_020.pt"), weights.split_transfer_state_dict(sd)[0], 48)
    model = TransferModel(_cfg(tmp_path, head, subtract, freeze))
    model.load_state_dict(sd)
    return model.cuda()


def _compat_module():
    compat = os.path.join(REPO, "compat")
    if "_repo" not in sys.modules:
        spec = importlib.util.spec_from_file_location("_repo", os.path.join(compat, "_repo.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        sys.modules["_repo"] = mod
    spec = importlib.util.spec_from_file_location("compat_train_thermompnn", os.path.join(compat, "train_thermompnn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _loss(pred, muts):
    return torch.stack([F.mse_loss(p["ddG"], m.ddG.cuda()) for p, m in zip(pred, muts) if m is not None and m.ddG is not None]).mean()


class Split:
    """tmpnn_finetune_forward / tmpnn_finetune_backward called directly on one prepared protein."""

    def __init__(self, tr, prot):
        from thermompnn_amd.autograd import plan_for
        self.tr, self.p, self.lib = tr, prot, tr.lib
        self.plan = plan_for(tr.model)
        self.common = (prot.X, prot.S, prot.mask, prot.ridx, prot.cenc)
        sb = self.lib.tmpnn_finetune_saved_bytes(prot.L, prot.M, tr.n_final, int(tr.lightattn), tr.n_layers, tr._cdims)
        cb = self.lib.tmpnn_finetune_scratch_bytes(prot.L, prot.M, tr.n_final, int(tr.lightattn), tr.n_layers, tr._cdims)
        assert sb > 0 and cb > 0
        self.saved = torch.empty(sb, dtype=torch.uint8, device="cuda")
        self.scratch = torch.empty(cb, dtype=torch.uint8, device="cuda")

    def _head(self):
        from thermompnn_amd.train import _ptr
        p = self.p
        return (*[_ptr(t) for t in self.common], p.L, _ptr(p.pos), _ptr(p.mut), _ptr(p.wt))

    def forward(self, p_mpnn, p_head, seed, step, slab=None):
        from thermompnn_amd._lib import check
        from thermompnn_amd.train import _ptr, _stream
        p, tr = self.p, self.tr
        pred = torch.empty(p.M, dtype=torch.float32, device="cuda")
        check(self.lib.tmpnn_finetune_forward(*self._head(), p.M, tr.n_final, int(tr.lightattn), tr.n_layers, tr._cdims, int(tr.subtract),
                                              _ptr(tr.slab if slab is None else slab), tr.numel, p_mpnn, p_head, None, None, None, seed,
                                              step, _ptr(pred), None, None, _ptr(self.saved), self.saved.numel(), _stream()))
        return pred

    def backward(self, p_mpnn, p_head, seed, step, dpred, mpnn_grads=1, slab=None):
        from thermompnn_amd._lib import check
        from thermompnn_amd.train import _ptr, _stream
        p, tr = self.p, self.tr
        grads = torch.zeros(tr.numel, dtype=torch.float32, device="cuda")
        dpred = dpred.float().cuda().contiguous()
        check(self.lib.tmpnn_finetune_backward(*self._head(), p.M, tr.n_final, int(tr.lightattn), tr.n_layers, tr._cdims, int(tr.subtract),
                                               _ptr(tr.slab if slab is None else slab), tr.numel, p_mpnn, p_head, None, None, seed, step,
                                               _ptr(dpred), _ptr(grads), mpnn_grads, _ptr(self.saved), self.saved.numel(),
                                               _ptr(self.scratch), self.scratch.numel(), _stream()))
        return grads


def _all_mutants(tr, pdb, muts):
    """A Protein over every non-None mutant (what the autograd path sees), targets 0 where unlabelled."""
    from thermompnn_amd.datasets import Mutation
    filled = [None if m is None else Mutation(m.position, m.wildtype, m.mutation, m.ddG if m.ddG is not None else torch.tensor([0.0]),
                                             m.pdb) for m in muts]
    return tr.prepare([(pdb, filled)])[0]


def _check_against_golden(g, tag, model, names):
    for name in names:
        grad = dict(model.named_parameters())[name].grad
        assert grad is not None, name
        dev = grad.reshape(-1).double().cpu().numpy()
        if f"{tag}|{name}|full" in g:
            ref = g[f"{tag}|{name}|full"].astype(np.float64)
            gmax = float(np.abs(ref).max())
            assert float(np.abs(dev - ref).max()) <= 1e-4 * gmax or float(np.abs(dev - ref).max()) <= 1e-12, (tag, name)
        else:
            idx, sign = _golden_sample_index(name, dev.size)
            gmax = float(g[f"{tag}|{name}|absmax"])
            assert abs(float(np.abs(dev).max()) - gmax) <= 1e-4 * gmax, (tag, name)
            assert float(np.abs(dev[idx] - g[f"{tag}|{name}|val"]).max()) <= 1e-4 * gmax, (tag, name)
            sumsq = float(g[f"{tag}|{name}|sumsq"])
            assert abs(float((dev * dev).sum()) - sumsq) <= 1e-4 * sumsq + 1e-20, (tag, name)
            assert abs(float((dev * sign).sum()) - float(g[f"{tag}|{name}|dot"])) <= 1e-4 * np.sqrt(dev.size * sumsq) + 1e-12, (tag, name)


def test_loss_backward_matches_the_reference_golden(tmp_path):
    """tests/golden/finetune_2OCJ_A.npz through the user's snippet: eval mode against `ones`, ProteinMPNN's dropout from the golden's
    (seed, step) against `drawn`."""
    from thermompnn_amd.autograd import dropout_key
    from thermompnn_amd.datasets import Mutation
    from thermompnn_amd.finetune import slab_shapes
    from thermompnn_amd.pdb_io import alt_parse_PDB
    g = load_golden("finetune_2OCJ_A")
    pdb = alt_parse_PDB(os.path.join(GOLDEN, "2OCJ.pdb"), ["A"])
    muts = [Mutation(int(p), AA20[w], AA20[m], None if np.isnan(t) else torch.tensor([float(t)]), "2OCJ")
            for p, w, m, t in zip(g["positions"], g["wildtype"], g["mutation"], g["targets"])]
    model = _model(tmp_path)
    model.differentiable = True
    names = list(slab_shapes(model.hidden_dims, 2, True))
    for tag in ("ones", "drawn"):
        model.zero_grad(set_to_none=True)
        if tag == "ones":
            model.eval()
            pred, second = model(pdb, muts)
        else:
            model.train()
            model.light_attention.eval()
            with dropout_key(int(g["seed"]), int(g["step"])):
                pred, second = model(pdb, muts)
        assert second is None and len(pred) == len(muts)
        assert all(p["ddG"].shape == (1,) and p["ddG"].requires_grad for p in pred)
        loss = _loss(pred, muts)
        loss.backward()
        ref_loss = float(g[f"{tag}_loss"])
        assert abs(float(loss.detach()) - ref_loss) <= 1e-6 * abs(ref_loss), (tag, float(loss.detach()), ref_loss)
        _check_against_golden(g, tag, model, names)
        assert model.prot_mpnn.W_out.weight.grad is None and model.prot_mpnn.W_out.bias.grad is None


SPLIT_CASES = CASES + [("2OCJ_A_gap", RELEASED, True, True), ("msk_L40", RELEASED, True, True), ("syn_L17", RELEASED, True, True)]


@pytest.mark.parametrize("case,head,subtract,dropout", SPLIT_CASES,
                         ids=[f"{c[0]}-nf{c[1]['num_final_layers']}-la{int(c[1]['lightattn'])}" for c in SPLIT_CASES])
def test_split_forward_backward_equals_the_fused_step_bit_for_bit(tmp_path, case, head, subtract, dropout):
    _split_equals_fused(tmp_path, case, head, subtract)


# the heavy draws ("hot": matrices x 3, biases x 5, LayerNorm gamma in [-2, 2]): (case, head, subtract, style, weight seed)
HOT_SPLIT_CASES = [("msk_L40", RELEASED, True, "hot", 0), ("syn_L17", NF0, True, "hot", 2)]


@pytest.mark.parametrize("case,head,subtract,style,seed", HOT_SPLIT_CASES, ids=[f"{c[0]}-nf{c[1]['num_final_layers']}-{c[3]}{c[4]}"
                                                                                for c in HOT_SPLIT_CASES])
def test_split_forward_backward_equals_the_fused_step_bit_for_bit_on_hot_weights(tmp_path, case, head, subtract, style, seed):
    _split_equals_fused(tmp_path, case, head, subtract, style, seed)


def _split_equals_fused(tmp_path, case, head, subtract, style="xavier", seed=0):
    from thermompnn_amd.finetune import MPNNTrainer
    model = _model(tmp_path, head, subtract, seed=seed, style=style)
    tr = MPNNTrainer(model, seed=7)
    pdb = _pdb(case, tmp_path)
    prot = tr.prepare([(pdb, _case_mutants(case, pdb))])[0]
    ph = 0.25 if head["lightattn"] else 0.0
    seed, step = 7, 3
    pred_f = torch.empty(prot.M, dtype=torch.float32, device="cuda")
    tr.grad.zero_()
    tr.forward_backward(prot, pred_out=pred_f, step=step, p_mpnn=0.1, p_head=ph)
    sp = Split(tr, prot)
    pred = sp.forward(0.1, ph, seed, step)
    torch.cuda.synchronize()
    assert torch.equal(pred, pred_f), float((pred - pred_f).abs().max())
    pn, tn = pred.cpu().numpy(), prot.target.cpu().numpy()
    dpred = torch.from_numpy((np.float32(2) * (pn - tn)) * (np.float32(1) / np.float32(prot.M)))
    saved0 = sp.saved.clone()
    g1 = sp.backward(0.1, ph, seed, step, dpred)
    g2 = sp.backward(0.1, ph, seed, step, dpred)
    torch.cuda.synchronize()
    assert torch.equal(sp.saved, saved0), "the backward wrote the saved buffer"
    diff = (g1 != tr.grad).nonzero()
    assert diff.numel() == 0, (diff[:5].tolist(), [k for k, o in tr.offsets.items() if o <= int(diff[0])][-1])
    assert torch.equal(g1, g2)


def test_loss_backward_on_a_gapped_chain_matches_the_float64_restatement(tmp_path):
    """TransferModel.differentiable on 2OCJ chain A with residue 120 missing its N (position 24, mask 0, mutants on it) and residues
    150-152 missing ('-' at 54-56): every .grad against restate() on the device's own k-NN graph."""
    from thermompnn_amd.finetune import MPNNTrainer
    model = _model(tmp_path)
    model.differentiable = True
    model.eval()
    pdb = _pdb("2OCJ_A_gap", tmp_path)
    muts = _mutants(pdb, 40, seed=3, with_none=False, at=(24, 24, 53, 57))
    pred, _ = model(pdb, muts)
    loss = _loss(pred, muts)
    loss.backward()
    tr = MPNNTrainer(model)
    prot = tr.prepare([(pdb, muts)])[0]
    assert float(prot.mask[24]) == 0.0 and int((prot.pos == 24).sum()) >= 2 and int((prot.S == 20).sum()) == 3
    E_idx = torch.empty((prot.L, 48), dtype=torch.int32, device="cuda")
    tr.forward_backward(prot, p_mpnn=0.0, p_head=0.0, E_idx_out=E_idx)
    torch.cuda.synchronize()
    ones = [np.ones((prot.L * (48 if s < 9 and s % 3 == 2 else 1), 128), np.float32) for s in range(15)]
    ref_loss, ref, _ = restate(model.state_dict(), list(tr.shapes), prot, E_idx.cpu().numpy(), ones, None, 2, True, True)
    assert abs(float(loss.detach()) - ref_loss) <= 1e-5 * max(abs(ref_loss), 1e-3), (float(loss.detach()), ref_loss)
    params = dict(model.named_parameters())
    # the '-' positions (token 20) are masked and no unmasked row of this chain has them among its 48 nearest: W_s[20] gets nothing
    assert float(ref["prot_mpnn.W_s.weight"][20].abs().max()) == 0.0 == float(params["prot_mpnn.W_s.weight"].grad[20].abs().max())
    for k in tr.shapes:
        g, r = params[k].grad.cpu().double(), ref[k]
        gmax, err = float(r.abs().max()), float((g - r).abs().max())
        assert err <= 1e-4 * gmax or err <= 1e-12, (k, err, gmax)
    assert model.prot_mpnn.W_out.weight.grad is None


def test_arbitrary_upstream_gradient_and_finite_differences(tmp_path):
    from thermompnn_amd.finetune import MPNNTrainer
    model = _model(tmp_path)
    model.differentiable = True
    model.eval()
    pdb = _pdb("syn_L40", tmp_path)
    muts = _mutants(pdb, 30, with_none=False)
    c = torch.from_numpy(np.random.default_rng(4).normal(size=len(muts)).astype(np.float32)).cuda()

    def objective():
        pred, _ = model(pdb, muts)
        return (torch.cat([p["ddG"] for p in pred]) * c).sum()

    objective().backward()
    tr = MPNNTrainer(model)
    prot = _all_mutants(tr, pdb, muts)
    sp = Split(tr, prot)
    sp.forward(0.0, 0.0, 0, 0)
    want = sp.backward(0.0, 0.0, 0, 0, c)
    params = dict(model.named_parameters())
    for k in tr.shapes:
        o, n = tr.offsets[k], params[k].numel()
        assert torch.equal(params[k].grad.reshape(-1), want[o:o + n]), k
    for name in ("ddg_out.weight", "prot_mpnn.W_e.weight"):
        p = params[name]
        flat_grad = p.grad.reshape(-1)
        i = int(flat_grad.abs().argmax())
        h = 2e-3 * max(1.0, float(p.detach().reshape(-1)[i].abs()))       # truncation ~h^2, fp32 noise ~1e-6 / h
        base = float(p.detach().reshape(-1)[i])
        vals = []
        for s in (1.0, -1.0):
            with torch.no_grad():
                p.view(-1)[i] = base + s * h
            vals.append(float(objective().detach()))
        with torch.no_grad():
            p.view(-1)[i] = base
        fd = (vals[0] - vals[1]) / (2 * h)
        g = float(flat_grad[i])
        assert abs(fd - g) <= 1e-2 * abs(g), (name, fd, g)


def test_arbitrary_upstream_gradient_matches_the_restatement_on_hot_weights(tmp_path):
    """The objective of test_arbitrary_upstream_gradient_and_finite_differences, sum(pred * c) through loss.backward(), from the hot
    draw (seed 0), against restate() with the same upstream gradient on the device's graph: the objective within 1e-5 relative and
    every .grad within 1e-4 x max|g|, the fine-tune tests' lines. The restatement in float32 alone is at 1.4e-6 resp. 5.0e-6 on this
    case (tests/test_train_weights_host.py, the "upstream" case). First passing run on the MI355X: objective 3.63e-6 relative,
    worst gradient 4.15e-6 of max|g| (ddg_out.weight)."""
    from thermompnn_amd.finetune import MPNNTrainer
    case, head, subtract, style, seed = UPSTREAM_CASE
    model = _model(tmp_path, head, subtract, seed=seed, style=style)
    model.differentiable = True
    model.eval()
    pdb = _pdb(case, tmp_path)
    muts = _mutants(pdb, 30, with_none=False)
    c = torch.from_numpy(np.random.default_rng(4).normal(size=len(muts)).astype(np.float32))
    pred, _ = model(pdb, muts)
    objective = (torch.cat([p["ddG"] for p in pred]) * c.cuda()).sum()
    objective.backward()
    tr = MPNNTrainer(model)
    prot = _all_mutants(tr, pdb, muts)
    assert prot.M == len(muts)
    L, K = prot.L, min(48, prot.L)
    E_idx = torch.empty((L, K), dtype=torch.int32, device="cuda")
    tr.forward_backward(prot, p_mpnn=0.0, p_head=0.0, E_idx_out=E_idx)
    torch.cuda.synchronize()
    ones = [np.ones((L * (K if s < 9 and s % 3 == 2 else 1), 128), np.float32) for s in range(15)]
    ref_obj, ref, _ = restate(model.state_dict(), list(tr.shapes), prot, E_idx.cpu().numpy(), ones, None, 2, True, subtract, upstream=c)
    params = dict(model.named_parameters())
    ratio = {k: float((params[k].grad.cpu().double() - r).abs().max()) / float(r.abs().max()) for k, r in ref.items()
             if float(r.abs().max()) > 1e-12}
    print(f"hot upstream: objective {ref_obj:.5g} rel. error {abs(float(objective.detach()) - ref_obj) / abs(ref_obj):.3g}, worst gradient "
          f"error / max|g| {max(ratio.values()):.3g}", max(ratio, key=ratio.get))
    assert abs(float(objective.detach()) - ref_obj) <= 1e-5 * max(abs(ref_obj), 1e-3)
    for k in tr.shapes:
        g, r = params[k].grad.cpu().double(), ref[k]
        gmax, err = float(r.abs().max()), float((g - r).abs().max())
        assert err <= 1e-4 * gmax or err <= 1e-12, (k, err, gmax)
    assert float(ref["prot_mpnn.W_e.weight"].abs().max()) > 0.0 and model.prot_mpnn.W_out.weight.grad is None


def test_frozen_encoder_gets_no_grad_and_head_grads_equal_the_split_backward(tmp_path):
    from thermompnn_amd.finetune import MPNNTrainer
    model = _model(tmp_path, freeze=True)
    assert not any(p.requires_grad for p in model.prot_mpnn.parameters())
    model.differentiable = True
    model.light_attention.eval()
    pdb = _pdb("2OCJ_A", tmp_path)
    muts = _mutants(pdb, 50)
    pred, _ = model(pdb, muts)
    _loss(pred, muts).backward()
    assert all(p.grad is None for p in model.prot_mpnn.parameters())
    tr = MPNNTrainer(model)
    prot = _all_mutants(tr, pdb, muts)
    sp = Split(tr, prot)
    got = sp.forward(0.0, 0.0, 0, 0)
    live = [m for m in muts if m is not None]
    assert torch.equal(got, torch.cat([p["ddG"] for p in pred if p is not None]).detach())
    pv = got.clone().requires_grad_(True)                      # dL/dpred with torch's own arithmetic
    lv = torch.stack([F.mse_loss(pv[i:i + 1], m.ddG.cuda()) for i, m in enumerate(live) if m.ddG is not None]).mean()
    dpred, = torch.autograd.grad(lv, pv)
    full = sp.backward(0.0, 0.0, 0, 0, dpred, mpnn_grads=1)
    params = dict(model.named_parameters())
    for k in tr.shapes:
        if k.startswith("prot_mpnn."):
            continue
        o = tr.offsets[k]
        assert torch.equal(params[k].grad.reshape(-1), full[o:o + params[k].numel()]), k


def test_two_proteins_summed_before_one_backward_equal_two_backwards(tmp_path):
    model = _model(tmp_path)
    model.differentiable = True
    model.eval()
    items = [(p, _mutants(p, 24, seed=i)) for i, p in enumerate((_pdb("syn_L40", tmp_path), _pdb("syn_L56", tmp_path)))]
    losses = [_loss(model(p, m)[0], m) for p, m in items]
    (losses[0] + losses[1]).backward()
    once = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
    model.zero_grad(set_to_none=True)
    for p, m in items:
        _loss(model(p, m)[0], m).backward()
    twice = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
    assert set(once) == set(twice) and len(once) == len(list(model.parameters())) - 2        # all but W_out
    for k in once:
        assert torch.equal(once[k], twice[k]), k


def test_a_torch_optimiser_loop_matches_mpnn_trainer(tmp_path):
    from thermompnn_amd import weights
    from thermompnn_amd.finetune import MPNNTrainer
    training = dict(learn_rate=1e-3, mpnn_learn_rate=1e-4)
    sd = weights.synthetic_state_dict(0, head=RELEASED)
    ref_model = _model(tmp_path)
    pl = _compat_module().TransferModelPL(_cfg(tmp_path, training=training))
    pl.model.load_state_dict(sd)
    pl.cuda()
    assert pl.model.differentiable
    pl.eval()
    items = []
    for i, case in enumerate(("syn_L40", "syn_L48", "2OCJ_A")):
        pdb = _pdb(case, tmp_path)
        items.append((pdb, _mutants(pdb, 30, seed=i, with_none=False)))   # every mutant labelled: the trainer sees the same M
    out = pl.configure_optimizers()
    opt = out if isinstance(out, torch.optim.Optimizer) else out["optimizer"]
    tr = MPNNTrainer(ref_model, learn_rate=1e-3, mpnn_learn_rate=1e-4, p_mpnn=0.0, p_head=0.0)
    prots = [tr.prepare([it])[0] for it in items]
    for step in range(5):
        k = step % 3
        opt.zero_grad()
        loss = pl.training_step([items[k]], step)
        loss.backward()
        opt.step()
        tr.grad.zero_()
        tr.step(prots[k])
    params = dict(pl.model.named_parameters())
    for k in tr.shapes:
        got, want = params[k].detach(), tr.tensor(k)
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-6), (k, float((got - want).abs().max()))
    assert torch.equal(params["prot_mpnn.W_out.weight"].detach().cpu(), sd["prot_mpnn.W_out.weight"])
    tr.write_back()
    ref_model.eval()
    pl.eval()
    for pdb, muts in items:
        with torch.no_grad():
            got = torch.cat([p["ddG"] for p in pl.model(pdb, muts)[0] if p is not None])
            want = torch.cat([p["ddG"] for p in ref_model(pdb, muts)[0] if p is not None])
        assert not got.requires_grad
        assert float((got - want).abs().max()) <= 1e-4


def test_no_grad_inference_sees_the_weights_after_an_optimiser_step(tmp_path):
    model = _model(tmp_path)
    model.differentiable = True
    model.eval()
    pdb = _pdb("syn_L40", tmp_path)
    muts = _mutants(pdb, 20, with_none=False)
    model.precision = "fp32"
    with torch.no_grad():
        before = torch.cat([p["ddG"] for p in model(pdb, muts)[0]])
    key = model._engine_key
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    _loss(model(pdb, muts)[0], muts).backward()
    opt.step()
    with torch.no_grad():
        after = torch.cat([p["ddG"] for p in model(pdb, muts)[0]])
    assert model._engine_key != key                               # the engine was rebuilt from the stepped weights
    grad_path = torch.cat([p["ddG"] for p in model(pdb, muts)[0]]).detach()
    assert float((after - before).abs().max()) > 1e-5
    assert float((after - grad_path).abs().max()) <= 1e-4


def test_default_path_is_untouched_and_dropout_follows_the_submodules(tmp_path):
    from thermompnn_amd.autograd import dropout_key
    from thermompnn_amd.datasets import ALPHABET
    from thermompnn_amd.finetune import MPNNTrainer
    model = _model(tmp_path)
    model.train()
    pdb = _pdb("syn_L48", tmp_path)
    muts = _mutants(pdb, 30)
    pred, _ = model(pdb, muts)                                   # differentiable left False: today's path
    live = [p["ddG"] for p in pred if p is not None]
    assert not any(v.requires_grad for v in live)
    table = model.ssm_table(pdb)
    want = torch.stack([table[m.position, ALPHABET.index(m.mutation)] for m in muts if m is not None])
    assert torch.equal(torch.cat(live), want)
    assert model(pdb, [None, None]) == ([None, None], None)
    model.differentiable = True
    assert model(pdb, [None, None]) == ([None, None], None)
    with dropout_key(3, 1):
        a = torch.cat([p["ddG"] for p in model(pdb, muts)[0] if p is not None])
        b = torch.cat([p["ddG"] for p in model(pdb, muts)[0] if p is not None])
    with dropout_key(3, 2):
        c = torch.cat([p["ddG"] for p in model(pdb, muts)[0] if p is not None])
    assert a.requires_grad and torch.equal(a, b) and not torch.equal(a, c)
    model.prot_mpnn.eval()
    with dropout_key(3, 1):
        d = torch.cat([p["ddG"] for p in model(pdb, muts)[0] if p is not None]).detach()
    tr = MPNNTrainer(model)
    sp = Split(tr, _all_mutants(tr, pdb, muts))
    assert torch.equal(d, sp.forward(0.0, 0.25, 3, 1))          # only the ProteinMPNN sites switched off
    assert torch.equal(a.detach(), sp.forward(0.1, 0.25, 3, 1))
    assert not torch.equal(d, sp.forward(0.0, 0.0, 3, 1))
