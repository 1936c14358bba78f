"""Drop-in for the reference's pipelines.py (the TLC-GNN link-prediction harness).

  train :10-18, test :20-40, weights_init :42-46, setup_seed :49-53, fit = the epoch loop of :111-126;
  train_forward = the forward of train() alone.

The reference's `train()` / `test()` are closures over the module-level `model`, `data`, `optimizer`; here they take them as
arguments.  Everything between the arguments and the returned numbers is the reference's: encode once, decode per split,
binary cross-entropy, roc_auc_score / average_precision_score on the host.  The forward itself runs on the HIP kernels behind
baselines/TLCGNN.py (Net.encode / Net.decode).  test(..., metrics="device") / fit(..., metrics="device") score the splits on the
device instead (metrics.py, csrc/lp_metrics.hip); the default stays the reference's sklearn path."""
import numpy as np
import torch
import torch.nn.functional as F


def weights_init(m):
    """:42-46  xavier_normal_ on every nn.Linear weight, zero bias (`model.apply(weights_init)`, :108)."""
    if isinstance(m, torch.nn.Linear):
        torch.nn.init.xavier_normal_(m.weight)
        if m.bias is not None:
            torch.nn.init.constant_(m.bias, 0)


def setup_seed(seed):
    """:49-53"""
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)


def train_forward(model, data):
    """The forward of train() (:11-15): model.train(), encode, decode('train') with its np.random.randint negatives, BCE.
    Returns (x, y, loss); the whole step, with loss.backward() / optimizer.step() (:16-17), is train().
    Training mode draws dropout masks, which the HIP encoder applies through torch's RNG (F.dropout in Net.encode)."""
    model.train()
    with torch.no_grad():
        emb = model.encode(data)
        x, y = model.decode(data, emb)
        loss = F.binary_cross_entropy(x, y)
    return x, y, loss


def train(model, data, optimizer):
    """:10-18: model.train(), zero_grad, encode, decode('train') with its np.random.randint negatives, BCE, backward, step;
    returns the predictions x.  The forward is the one of train_forward (same kernels, same draws, same x); the backward runs
    on the HIP kernels of lp_backward.hip through autograd.GcnLayer / autograd.LpDecode."""
    model.train()
    optimizer.zero_grad()
    emb = model._encode_train(data)
    x, y = model._decode_train(data, emb)
    loss = F.binary_cross_entropy(x, y)
    loss.backward()
    optimizer.step()
    return x


def train_curvature(model, data, optimizer, images):
    """The step of train() with a LEARNED image table: the image rows of the step's pairs come from `images()` -- a
    `topo.VicinityImages` over the training part of data.total_edges (its first train_pos + train_neg rows, or the whole list) --
    instead of model.PI, so loss.backward() also reaches `images.kappa`, the graph's curvature.  `optimizer` holds
    the model's parameters and images.kappa (one optimizer or a parameter group).  The negatives are drawn as Net.decode draws them
    (np.random.randint over the same fixed pair list); the stored table model.PI takes no part in the step.  Returns the predictions x."""
    from . import autograd as ag
    model.train()
    optimizer.zero_grad()
    emb = model._encode_train(data)
    dev = emb.device
    _, pairs_all = model._tables(data, dev)
    if not isinstance(pairs_all, torch.Tensor):
        raise TypeError("train_curvature: a streamed pair list (pi_cache.LazyPairList) is not taken: the images need the fixed list")
    tp, tn = data.train_pos, data.train_neg
    n_img = images.structure.n_pairs
    if n_img < tp + tn or not torch.equal(images.structure.pairs[:tp + tn], pairs_all[:tp + tn]):
        raise ValueError("train_curvature: images should be built over data.total_edges[:train_pos + train_neg] (or the whole list)")
    index = np.random.randint(0, tn, tp)                               # same RNG call as TLCGNN.py:31
    idx = torch.cat((torch.arange(tp, device=dev), tp + torch.from_numpy(index).to(dev)))
    y = data.total_edges_y[idx.to(data.total_edges_y.device)].float()
    table, _ = images()
    # (table[idx]: its backward is index_put_(accumulate=True), which sorts -- repeated negatives add up in a fixed order)
    pi = table[idx].to(torch.float32)
    x = ag.lp_decode(emb, pairs_all[idx].contiguous(), pi, model.linear_1.weight, model.linear_1.bias, model.linear.weight, model.linear.bias)
    loss = F.binary_cross_entropy(x, y.to(x.device))
    loss.backward()
    optimizer.step()
    return x


def fit(model, data, optimizer, total_epochs=2000, wait_total=200, metrics="sklearn"):
    """The epoch loop of :111-126: train, then test; the test numbers of the best validation ROC-AUC (>=) are kept, and the loop
    stops after `wait_total` epochs without a better one -> (test_acc, test_roc, best_val_acc, best_val_roc, best_val_loss)
    (acc = average precision, as the reference names it).  metrics: passed to test()."""
    best_val_acc = test_acc = 0.0
    best_val_roc = test_roc = 0.0
    best_val_loss = np.inf
    wait_step = 0
    for epoch in range(1, total_epochs + 1):
        train(model, data, optimizer)
        val_loss, val_roc, val_acc, tmp_test_roc, tmp_test_acc = test(model, data, metrics=metrics)
        if val_roc >= best_val_roc:
            test_acc, test_roc = tmp_test_acc, tmp_test_roc
            best_val_acc, best_val_roc, best_val_loss = val_acc, val_roc, val_loss
            wait_step = 0
        else:
            wait_step += 1
            if wait_step == wait_total:
                break
    return test_acc, test_roc, best_val_acc, best_val_roc, best_val_loss


def test(model, data, metrics="sklearn"):
    """:20-40 -> [val BCE, val ROC-AUC, val AP, test ROC-AUC, test AP].

    metrics="sklearn" (default): the reference's path, predictions copied to the host, BCE on the CPU, sklearn's scores.
    metrics="device": both splits scored by one tlc_binary_rank_metrics call (two segments), the val BCE on the device, then one
    copy of the five numbers to the host.  Same list, order and types (a 0-dim float32 CPU tensor, then four floats)."""
    if metrics == "device":
        return _test_device(model, data)
    if metrics != "sklearn":
        raise ValueError("metrics must be 'sklearn' or 'device', not %r" % (metrics,))
    from sklearn.metrics import roc_auc_score, average_precision_score
    model.eval()
    accs = []
    with torch.no_grad():
        emb = model.encode(data)
        for split in ["val", "test"]:
            pred, y = model.decode(data, emb, type=split)
            pred, y = pred.cpu(), y.cpu()
            if split == "val":
                accs.append(F.binary_cross_entropy(pred, y))
            pred = pred.data.numpy()
            accs.append(roc_auc_score(y, pred))
            accs.append(average_precision_score(y, pred))
    return accs


def _test_device(model, data):
    from . import metrics, ops
    model.eval()
    with torch.no_grad():
        emb = model.encode(data)
        pv, yv = model.decode(data, emb, type="val")
        pt, yt = model.decode(data, emb, type="test")
        yv, yt = yv.to(pv.device), yt.to(pt.device)
        nv, nt = pv.numel(), pt.numel()
        auc, ap, n_pos, n_neg, status = ops.binary_rank_metrics(torch.cat([pv, pt]), torch.cat([yv, yt]), [0, nv, nv + nt])
        bce = F.binary_cross_entropy(pv, yv)
        # one copy to the host; the f32 BCE, the counts (< 2^31) and the status words are exact in float64
        v = torch.cat([bce.double().reshape(1), auc, ap, n_pos.double(), n_neg.double(), status.double()]).cpu()
    h = v.tolist()            # [bce, auc val, auc test, ap val, ap test, n_pos val, test, n_neg val, test, status val, test]
    for s, what in enumerate(["val", "test"]):
        metrics.check_status(int(h[9 + s]), "pipelines.test: %s split" % what)
        metrics.warn_single_class(int(h[5 + s]), int(h[7 + s]))
    return [v[0].float(), h[1], h[3], h[2], h[4]]
