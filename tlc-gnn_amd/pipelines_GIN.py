"""Drop-in for the reference's pipelines_GIN.py (node classification on PDGNN images, Knowledge_Distillation/ConvCurv_GIN.py).

  train :15-21, test :23-31, settings = the epoch budget of :51-56, loader_of :60-67, split_masks :101-116, fit = the epoch loop of
  :119-134 (Adam(lr=0.005, weight_decay=5e-4) is :118).

The reference's `train()` / `test()` are closures over the module-level `model`, `data`, `optimizer`; here they take them as
arguments.  The forward and backward of the two curvGN layers run on the HIP kernels of csrc/nc_curv.hip (autograd.CurvConv);
dropout, ELU, log_softmax and the NLL stay torch ops.  test() runs ONE forward: the forward is deterministic, so the reference's
second forward for the validation loss (:30) returns the same values."""
import random

import numpy as np
import torch
import torch.nn.functional as F


def loader_of(d_name):
    """:60-67"""
    if d_name in ('Cora', 'Citeseer', 'PubMed'):
        return 'Planetoid'
    if d_name in ('Computers', 'Photo'):
        return 'Amazon'
    if d_name in ('CS', 'Physics'):
        return 'Coauthor'
    return 'Synthesis'


def settings(d_name):
    """:51-56 -> (total_epochs, wait_total)."""
    if d_name == 'Photo' or d_name == 'Computers':
        return 500, 200
    return 200, 100


def split_masks(data, d_loader, rng=random):
    """:101-116 -> (train_mask, val_mask, test_mask), bool tensors on data.y's device.  Planetoid: the dataset's own masks; Amazon /
    Coauthor: the first 20 per class for training, the next 500 for validation, the last 1 000 for test; otherwise (:111-116) a
    shuffled index (rng.shuffle, the reference's random.shuffle) with 400 / 400 / 200."""
    y = data.y
    n = len(y)
    if d_loader == 'Planetoid':
        return data.train_mask.bool(), data.val_mask.bool(), data.test_mask.bool()
    index = np.arange(n)
    if d_loader == 'Coauthor' or d_loader == 'Amazon':
        train_len = 20 * int(y.max() + 1)
        train = index < train_len
        val = (index >= train_len) & (index < 500 + train_len)
        test = index >= n - 1000
    else:
        index = list(range(n))
        rng.shuffle(index)
        index = np.asarray(index)
        len_mul = int(1000 / 5)
        train = index < len_mul * 2
        val = (index >= len_mul * 2) & (index < len_mul * 4)
        test = index >= (n - len_mul)
    dev = y.device
    return tuple(torch.from_numpy(m).to(dev) for m in (train, val, test))


def train(model, data, optimizer, train_mask):
    """:15-21: model.train(), zero_grad, NLL of the train rows, backward (HIP), step."""
    model.train()
    optimizer.zero_grad()
    loss = F.nll_loss(model(data)[train_mask], data.y[train_mask])
    loss.backward()
    optimizer.step()
    return loss


def test(model, data, train_mask, val_mask, test_mask):
    """:23-31 -> [train_acc, val_acc, test_acc, val_loss] (accuracies as floats, the loss a 0-dim tensor)."""
    model.eval()
    with torch.no_grad():
        logits, accs = model(data), []
        for mask in [train_mask, val_mask, test_mask]:
            pred = logits[mask].max(1)[1]
            acc = pred.eq(data.y[mask]).sum().item() / mask.sum().item()
            accs.append(acc)
        accs.append(F.nll_loss(logits[val_mask], data.y[val_mask]))
    return accs


def fit(model, data, optimizer, train_mask, val_mask, test_mask, total_epochs=200, wait_total=100):
    """The epoch loop of :119-134: train, then test; the test accuracy of the best validation accuracy (>=) is kept, and the loop
    stops after `wait_total` epochs without one -> (test_acc, best_val_acc, best_val_loss, epochs run)."""
    best_val_acc = test_acc = 0.0
    best_val_loss = np.inf
    wait_step = 0
    epoch = 0
    for epoch in range(1, total_epochs + 1):
        train(model, data, optimizer, train_mask)
        train_acc, val_acc, tmp_test_acc, val_loss = test(model, data, train_mask, val_mask, test_mask)
        if val_acc >= best_val_acc:
            test_acc = tmp_test_acc
            best_val_acc = val_acc
            best_val_loss = val_loss
            wait_step = 0
        else:
            wait_step += 1
            if wait_step == wait_total:
                break
    return test_acc, best_val_acc, best_val_loss, epoch


def optimizer_for(model):
    """:118"""
    return torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=0.0005)
