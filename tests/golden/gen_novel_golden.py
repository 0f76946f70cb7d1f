#!/usr/bin/env python3
"""Generate tests/golden/novel_*.npz by running the REFERENCE's get_top_novel_predictions in place (build container only).

    python tests/golden/gen_novel_golden.py      # needs the reference checkout (as gen_golden.py); never on the GPU box

The reference's own ``train.get_top_novel_predictions`` (train.py:26-151) runs on its own ``model.Net`` through the
DGL stand-in, with a dataset namespace that provides what the function reads: ``association_matrix``, ``num_drug``,
``num_disease``, ``_generate_dec_graph`` (bound from ``DrugDataLoader``) and ``get_graph_data_for_training``.
Nothing from the reference is copied: only inputs, the ``state_dict``, the association matrix and the returned rows
are stored, as arrays.

At initialisation the decoder's scores all sit within ~1e-4 of one value, one ulp apart, so their order would be
rounding noise.  The decoder's weights are therefore redrawn at a larger scale, lin3 is rescaled so the first k + 1
logits span ~4 around 0 (where the sigmoid is steepest), and a draw is kept only when consecutive scores among the
first k + 1 differ by at least 1e-4: the order is then unambiguous at the tests' 1e-5.

  novel_top50.npz  90 x 70, k = 50 (5 000-pair batches: the function runs two)
  novel_all.npz    12 x 10, fewer novel pairs than k = 200: the reference returns all of them
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (installs the DGL stand-in, puts the reference on sys.path)

import train as ref_train  # noqa: E402  (imports as-is through the stand-in)

ref_dl, ref_model = gg.ref_dl, gg.ref_model
MIN_GAP = 1e-4


def _case(name, seed, n_drug, n_dis, k, extra_known):
    emb, agg, out_units, layers, nhid1 = 24, 48, 8, 3, 16
    for attempt in range(50):
        rng = np.random.default_rng(seed + 1000 * attempt)
        pairs, vals, enc = gg._build_enc(rng, n_drug, n_dis)
        drug_graph, dis_graph = gg._sim_adj(rng, n_drug, 4), gg._sim_adj(rng, n_dis, 4)
        drug_fg, dis_fg = gg._sim_adj(rng, n_drug, 4), gg._sim_adj(rng, n_dis, 4)
        drug_feat = th.nn.functional.normalize(th.from_numpy(rng.standard_normal((n_drug, emb)).astype(np.float32)))
        dis_feat = th.nn.functional.normalize(th.from_numpy(rng.standard_normal((n_dis, emb)).astype(np.float32)))
        # similarity rows on a 1/256 grid and decoder weights on a 2^-8 grid: exact in fp32, and they compress
        drug_sim = th.from_numpy((rng.integers(0, 256, (n_drug, n_drug)) / 256.0).astype(np.float32))
        dis_sim = th.from_numpy((rng.integers(0, 256, (n_dis, n_dis)) / 256.0).astype(np.float32))
        # every known association of the dataset: the training positives and further cells (other folds' positives)
        assoc = np.zeros((n_drug, n_dis), np.float32)
        assoc[pairs[0][vals > 0], pairs[1][vals > 0]] = 1.0
        assoc[rng.random((n_drug, n_dis)) < extra_known] = 1.0

        args = types.SimpleNamespace(rating_vals=[0, 1], src_in_units=emb, dst_in_units=emb, gcn_agg_units=agg,
                                     gcn_out_units=out_units, dropout=0.0, gcn_agg_accum="sum", model_activation="leaky",
                                     share_param=True, device="cpu", layers=layers, fdim_drug=n_drug, fdim_disease=n_dis,
                                     nhid1=nhid1, nhid2=out_units, attention_dropout=0.0, save_dir=None)
        th.manual_seed(seed + attempt)
        net = ref_model.Net(args)
        with th.no_grad():  # spread the scores (see the module docstring)
            for lin, scale in ((net.decoder.lin1, 0.6), (net.decoder.lin2, 0.25), (net.decoder.lin3, 0.5)):
                lin.weight.copy_(th.round(th.randn_like(lin.weight) * scale * 256) / 256)
                lin.bias.copy_(th.round(th.randn_like(lin.bias) * 0.1 * 256) / 256)

        graph_data = {"train_enc_graph": enc, "drug_graph": drug_graph, "drug_sim_features": drug_sim,
                      "drug_features": drug_feat, "disease_graph": dis_graph, "disease_sim_features": dis_sim,
                      "disease_features": dis_feat, "drug_feature_graph": drug_fg, "disease_feature_graph": dis_fg}
        ds = types.SimpleNamespace(association_matrix=assoc, num_drug=n_drug, num_disease=n_dis, _num_drug=n_drug,
                                   _num_disease=n_dis, _symm=True)
        ds._generate_dec_graph = types.MethodType(ref_dl.DrugDataLoader._generate_dec_graph, ds)
        ds.get_graph_data_for_training = lambda cv_idx: graph_data
        n_novel = int((assoc == 0).sum())
        with tempfile.TemporaryDirectory() as tmp:
            args.save_dir = tmp  # the function writes a CSV there
            s_all = ref_train.get_top_novel_predictions(args, net, ds, 0, top_k=n_novel)["score"].to_numpy(np.float64)
        # the logit is affine in lin3: stretch the first k + 1 over ~4 logits around 0, where sigmoid is steepest
        lg = np.log(s_all) - np.log1p(-s_all)
        top = lg[:min(k, n_novel) + 1]
        c = 4.0 / max(top[0] - top[-1], 1e-3)
        with th.no_grad():
            net.decoder.lin3.weight.mul_(c)
            net.decoder.lin3.bias.mul_(c).sub_(c * top[len(top) // 2])
        with tempfile.TemporaryDirectory() as tmp:
            args.save_dir = tmp
            df = ref_train.get_top_novel_predictions(args, net, ds, 0, top_k=k)
        scores = df["score"].to_numpy(np.float64)
        assert len(df) == min(k, n_novel)
        # the first k + 1 scores: one more call with k + 1
        with tempfile.TemporaryDirectory() as tmp:
            args.save_dir = tmp
            scores1 = ref_train.get_top_novel_predictions(args, net, ds, 0, top_k=k + 1)["score"].to_numpy(np.float64)
        if len(scores1) > 1 and (-np.diff(scores1)).min() >= MIN_GAP:
            break
        print("%s: attempt %d has a score gap below %g; redrawing" % (name, attempt, MIN_GAP))
    else:
        raise RuntimeError("no draw with distinct scores")
    gaps = -np.diff(scores1)
    assert gaps.min() >= MIN_GAP, gaps.min()
    assert np.array_equal(scores1[:len(scores)], scores)

    arrays = dict(n_drug=n_drug, n_dis=n_dis, emb=emb, agg_units=agg, out_units=out_units, layers=layers, nhid1=nhid1,
                  k=k, enc_drug=pairs[0].astype(np.int32), enc_dis=pairs[1].astype(np.int32),
                  enc_values=vals.astype(np.float32), drug_feat=drug_feat, dis_feat=dis_feat, drug_sim=drug_sim,
                  dis_sim=dis_sim, association=assoc.astype(np.uint8),
                  ref_drug_id=df["drug_id"].to_numpy(np.int64), ref_disease_id=df["disease_id"].to_numpy(np.int64),
                  ref_score=scores)
    for nm, adj in (("drug_graph", drug_graph), ("dis_graph", dis_graph), ("drug_fg", drug_fg), ("dis_fg", dis_fg)):
        arrays[nm + "_row"], arrays[nm + "_col"], arrays[nm + "_val"] = adj._indices()[0], adj._indices()[1], adj._values()
    for key, v in net.state_dict().items():
        arrays["sd_" + key] = v
    gg.save(name, **arrays)
    assert os.path.getsize(os.path.join(HERE, name + ".npz")) < 100 * 1024


if __name__ == "__main__":
    _case("novel_top50", 1100, 90, 70, 50, 0.02)
    _case("novel_all", 1200, 12, 10, 200, 0.6)
