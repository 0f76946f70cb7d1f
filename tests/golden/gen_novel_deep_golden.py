#!/usr/bin/env python3
"""Generate tests/golden/novel_deep1500.npz by running the REFERENCE's get_top_novel_predictions in place with a
``top_k`` beyond the on-chip limit (build container only).

    python tests/golden/gen_novel_deep_golden.py      # needs the reference checkout (as gen_golden.py); never on the GPU box

Set up exactly as gen_novel_golden.py (the reference's own function on its own ``model.Net`` through the DGL stand-in,
a dataset namespace with what the function reads, decoder weights redrawn at a larger scale and lin3 rescaled so that
the first k + 1 logits span ~4 around 0).  Nothing from the reference is copied: only inputs, the ``state_dict``, the
association matrix and the returned rows are stored, as arrays.

  novel_deep1500.npz  64 x 48, k = 1500

A 1e-4 gap between consecutive scores cannot be had at 1500 rows, so the order inside the list is compared through
the scores and only the SET is pinned: a draw is kept when at most ``MAX_NEAR`` of the reference's rows (on either side
of the cut) score within ``NEAR`` of its 1500th, the only rows whose membership fp32 rounding may decide.  The next
``N_NEXT`` rows after the 1500th are stored as well, so that a test can name the reference score of a pair just
outside the reference's list.
"""
import os
import tempfile
import types

import numpy as np
import torch as th

import gen_novel_golden as gn  # noqa: E402  (installs the DGL stand-in, puts the reference on sys.path)

gg, ref_train, ref_dl, ref_model = gn.gg, gn.ref_train, gn.ref_dl, gn.ref_model
NEAR = 2e-5
MAX_NEAR = 8
N_NEXT = 32


def _top(args, net, ds, k):
    with tempfile.TemporaryDirectory() as tmp:
        args.save_dir = tmp  # the function writes a CSV there
        return ref_train.get_top_novel_predictions(args, net, ds, 0, top_k=k)


def _case(name, seed, n_drug, n_dis, k, extra_known):
    emb, agg, out_units, layers, nhid1 = 24, 48, 8, 3, 16
    for attempt in range(50):
        rng = np.random.default_rng(seed + 1000 * attempt)
        pairs, vals, enc = gg._build_enc(rng, n_drug, n_dis)
        drug_graph, dis_graph = gg._sim_adj(rng, n_drug, 4), gg._sim_adj(rng, n_dis, 4)
        drug_fg, dis_fg = gg._sim_adj(rng, n_drug, 4), gg._sim_adj(rng, n_dis, 4)
        drug_feat = th.nn.functional.normalize(th.from_numpy(rng.standard_normal((n_drug, emb)).astype(np.float32)))
        dis_feat = th.nn.functional.normalize(th.from_numpy(rng.standard_normal((n_dis, emb)).astype(np.float32)))
        drug_sim = th.from_numpy((rng.integers(0, 256, (n_drug, n_drug)) / 256.0).astype(np.float32))
        dis_sim = th.from_numpy((rng.integers(0, 256, (n_dis, n_dis)) / 256.0).astype(np.float32))
        assoc = np.zeros((n_drug, n_dis), np.float32)
        assoc[pairs[0][vals > 0], pairs[1][vals > 0]] = 1.0
        assoc[rng.random((n_drug, n_dis)) < extra_known] = 1.0
        n_novel = int((assoc == 0).sum())
        assert n_novel >= k + N_NEXT, n_novel

        args = types.SimpleNamespace(rating_vals=[0, 1], src_in_units=emb, dst_in_units=emb, gcn_agg_units=agg,
                                     gcn_out_units=out_units, dropout=0.0, gcn_agg_accum="sum", model_activation="leaky",
                                     share_param=True, device="cpu", layers=layers, fdim_drug=n_drug, fdim_disease=n_dis,
                                     nhid1=nhid1, nhid2=out_units, attention_dropout=0.0, save_dir=None)
        th.manual_seed(seed + attempt)
        net = ref_model.Net(args)
        with th.no_grad():  # spread the scores (gen_novel_golden.py's module docstring)
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
        s_all = _top(args, net, ds, n_novel)["score"].to_numpy(np.float64)
        # the logit is affine in lin3: stretch the first k + 1 over ~4 logits around 0, where sigmoid is steepest
        lg = np.log(s_all) - np.log1p(-s_all)
        top = lg[:k + 1]
        c = 4.0 / max(top[0] - top[-1], 1e-3)
        with th.no_grad():
            net.decoder.lin3.weight.mul_(c)
            net.decoder.lin3.bias.mul_(c).sub_(c * top[len(top) // 2])
        df = _top(args, net, ds, k)
        scores = df["score"].to_numpy(np.float64)
        assert len(df) == k
        df_all = _top(args, net, ds, n_novel)
        s_all = df_all["score"].to_numpy(np.float64)
        near = int((np.abs(s_all - scores[-1]) <= NEAR).sum())  # the 1500th itself included
        if near <= MAX_NEAR and np.array_equal(s_all[:k], scores):
            break
        print("%s: attempt %d has %d rows within %g of the %d-th score; redrawing" % (name, attempt, near, NEAR, k))
    else:
        raise RuntimeError("no draw with few enough rows at the cut")
    assert int((np.abs(s_all - scores[-1]) <= NEAR).sum()) <= MAX_NEAR
    assert np.array_equal(df_all["drug_id"].to_numpy()[:k], df["drug_id"].to_numpy())
    assert np.array_equal(df_all["disease_id"].to_numpy()[:k], df["disease_id"].to_numpy())
    assert abs(s_all[k + N_NEXT - 1] - scores[-1]) > NEAR  # the stored rows reach past the near band
    nxt = df_all.iloc[k:k + N_NEXT]

    arrays = dict(n_drug=n_drug, n_dis=n_dis, emb=emb, agg_units=agg, out_units=out_units, layers=layers, nhid1=nhid1,
                  k=k, enc_drug=pairs[0].astype(np.int32), enc_dis=pairs[1].astype(np.int32),
                  enc_values=vals.astype(np.float32), drug_feat=drug_feat, dis_feat=dis_feat, drug_sim=drug_sim,
                  dis_sim=dis_sim, association=assoc.astype(np.uint8),
                  ref_drug_id=df["drug_id"].to_numpy(np.int16), ref_disease_id=df["disease_id"].to_numpy(np.int16),
                  ref_score=scores, ref_next_drug_id=nxt["drug_id"].to_numpy(np.int16),
                  ref_next_disease_id=nxt["disease_id"].to_numpy(np.int16), ref_next_score=nxt["score"].to_numpy(np.float64))
    for nm, adj in (("drug_graph", drug_graph), ("dis_graph", dis_graph), ("drug_fg", drug_fg), ("dis_fg", dis_fg)):
        arrays[nm + "_row"], arrays[nm + "_col"], arrays[nm + "_val"] = adj._indices()[0], adj._indices()[1], adj._values()
    for key, v in net.state_dict().items():
        arrays["sd_" + key] = v
    gg.save(name, **arrays)
    assert os.path.getsize(os.path.join(gn.HERE, name + ".npz")) < 100 * 1024


if __name__ == "__main__":
    _case("novel_deep1500", 1300, 64, 48, 1500, 0.02)
