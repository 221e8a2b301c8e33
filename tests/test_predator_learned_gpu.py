"""A learned Predator_APR run at a reduced budget (apr_amd/predator/lib/learned.py::train_and_test): 16 x 400-ray pairs,
3 training / 2 validation / 2 test pairs, one complement scan a side, EPOCHS epochs of the reference's train() body, then the
tester's epoch.

Measured on an MI355X: 5.2 s for the two runs (one: 2.6 s building the pairs, 1.15 s for the 12 training iterations, 0.57 s
for the five validation epochs, 0.02 s for the tester's epoch); mean training total per epoch 2.1235, 1.8686, 1.7583, 1.7209;
held-out validation circle_loss 1.6439 (untrained) -> 1.3740 after epoch 4.  The validation recall stays near 0.04 at this
budget, so the saliency weight stays 0.0 in every epoch, and no test pair registers within 5 degrees / 2 m (recall 0.0, the
six statistics NaN): twelve iterations do not make a matcher, the test checks the recipe's plumbing and its repeatability.
"""
import time

import numpy as np
import pytest
import torch

from apr_amd.predator.lib.learned import train_and_test
from apr_amd.predator.lib.validation import KEYS, saliency_weight

pytestmark = pytest.mark.gpu

EPOCHS = 4


def test_training_lowers_the_training_total_and_repeats_bit_for_bit(dev):
    t0 = time.perf_counter()
    kw = dict(n_train=3, n_val=2, n_test=2, epochs=EPOCHS, n_beams=16, n_azimuth=400, k=1, seed=0, n_points=1000,
              max_iteration=5000)
    a = train_and_test(dev, **kw)
    b = train_and_test(dev, **kw)
    first, last = a["train"][0]["total"], a["train"][-1]["total"]
    before, after = a["valid"][0]["circle_loss"], a["valid"][-1]["circle_loss"]
    print(f"{time.perf_counter() - t0:.1f} s for two runs; seconds of one: { {k: round(v, 2) for k, v in a['seconds'].items()} }")
    print(f"training total, epoch means: {[round(e['total'], 4) for e in a['train']]}")
    print(f"held-out circle_loss {before:.4f} (untrained) -> {after:.4f}; recall {[round(v['recall'], 3) for v in a['valid']]}; "
          f"w_saliency {a['w_saliency_history']}; test recall {a['test']['recall']}, errors {a['test']['errors']}")
    # two fresh runs: the same bits
    assert len(a["iterations"]) == EPOCHS * 3 and a["invalid"] == 0
    assert a["iterations"] == b["iterations"]
    assert len(a["valid_records"]) == EPOCHS + 1
    for ra, rb in zip(a["valid_records"], b["valid_records"]):
        assert ra.tobytes() == rb.tobytes() and ra.shape[0] == 2
    assert a["test_records"].tobytes() == b["test_records"].tobytes() and a["test_records"].shape[0] == 2
    assert a["w_saliency_history"] == b["w_saliency_history"] and a["valid"] == b["valid"]
    # everything is finite
    assert all(np.isfinite(v) for it in a["iterations"] for v in it.values())
    assert all(np.isfinite(r).all() for r in a["valid_records"]) and np.isfinite(a["test_records"]).all()
    assert all(np.isfinite(d[k]) for d in a["valid"] for k in KEYS)
    # the optimiser works, and what it learned carries over to the held-out pairs
    assert last < first, (first, last)
    assert after < before, (before, after)
    # the recipe's switch: the weight an epoch's validation sets is what the next epoch trains with
    assert len(a["w_saliency_history"]) == EPOCHS
    for e in range(EPOCHS):
        assert a["w_saliency_history"][e] == saliency_weight(a["valid"][e + 1]["recall"])
    assert a["best_loss"][0] == min(d["circle_loss"] for d in a["valid"][1:])
    assert a["best_recall"][0] == max(d["recall"] for d in a["valid"][1:])
    assert 0.0 <= a["test"]["recall"] <= 1.0
