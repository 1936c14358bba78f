"""Drop-in for the reference's pipelines.py (the TLC-GNN link-prediction harness).

  train :10-18, test :20-40, weights_init :42-46, setup_seed :49-53, fit = the epoch loop of :111-126;
  train_forward = the forward of train() alone.

The reference's `train()` / `test()` are closures over the module-level `model`, `data`, `optimizer`; here they take them as
arguments.  Everything between the arguments and the returned numbers is the reference's: encode once, decode per split,
binary cross-entropy, roc_auc_score / average_precision_score on the host.  The forward itself runs on the HIP kernels behind
baselines/TLCGNN.py (Net.encode / Net.decode)."""
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


def fit(model, data, optimizer, total_epochs=2000, wait_total=200):
    """The epoch loop of :111-126: train, then test; the test numbers of the best validation ROC-AUC (>=) are kept, and the loop
    stops after `wait_total` epochs without a better one -> (test_acc, test_roc, best_val_acc, best_val_roc, best_val_loss)
    (acc = average precision, as the reference names it)."""
    best_val_acc = test_acc = 0.0
    best_val_roc = test_roc = 0.0
    best_val_loss = np.inf
    wait_step = 0
    for epoch in range(1, total_epochs + 1):
        train(model, data, optimizer)
        val_loss, val_roc, val_acc, tmp_test_roc, tmp_test_acc = test(model, data)
        if val_roc >= best_val_roc:
            test_acc, test_roc = tmp_test_acc, tmp_test_roc
            best_val_acc, best_val_roc, best_val_loss = val_acc, val_roc, val_loss
            wait_step = 0
        else:
            wait_step += 1
            if wait_step == wait_total:
                break
    return test_acc, test_roc, best_val_acc, best_val_roc, best_val_loss


def test(model, data):
    """:20-40 -> [val BCE, val ROC-AUC, val AP, test ROC-AUC, test AP]."""
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
