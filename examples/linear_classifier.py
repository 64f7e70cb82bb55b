"""A two-layer perceptron trained with AdamW; every array is resident on the MI355X and a layer is one launch forward.

    h      = dnn_linear_forward(x, W1, b1, "tanh")              x . W1^T + b1 and the tanh in one kernel
    logits = dnn_linear_forward(h, W2, b2)
    loss, dlogits = dnn_cross_entropy(logits, labels, "mean", with_grad=True)
    dW2, dh, db2 = dnn_linear_backward(h, dlogits, W2, bias=True)
    dW1, _, db1  = dnn_linear_backward(x, dh, W1, out=h, activation="tanh", bias=True, need_dx=False)
                                                                 the first layer asks for no input gradient and pays for none
    opt.step([dW1, db1, dW2, db2])                               optim.AdamW: one launch for the four parameters

No array is ever turned around and no bare product is taken: the layer reads x, W and dy where they lie.

`python examples/linear_classifier.py [samples] [steps]` prints the loss; main() asserts that it falls.  tests/test_gpu_linear.py
runs a small instance."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from numpower_amd import optim  # noqa: E402
from numpower_amd.ndarray import NDArray as nd  # noqa: E402

LR = 0.02
WEIGHT_DECAY = 0.01


def make_problem(samples: int, features: int, classes: int, seed: int = 0):
    """-> X (samples, features) float32 around one of `classes` centres, labels (samples,) int"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((classes, features)).astype(np.float32) * 2.0
    labels = rng.integers(0, classes, samples)
    return (centres[labels] + 0.5 * rng.standard_normal((samples, features))).astype(np.float32), labels


def init_params(features: int, hidden: int, classes: int, seed: int = 1):
    """-> [W1 (hidden, features), b1 (hidden), W2 (classes, hidden), b2 (classes)] on the GPU"""
    rng = np.random.default_rng(seed)
    host = [rng.standard_normal((hidden, features)) / np.sqrt(features), np.zeros(hidden),
            rng.standard_normal((classes, hidden)) / np.sqrt(hidden), np.zeros(classes)]
    return [nd.array(a.astype(np.float32)).gpu() for a in host]


def _value(loss):
    return float(loss) if isinstance(loss, (int, float, np.floating)) else float(np.asarray(loss.cpu().numpy()).reshape(-1)[0])


def gradients(gX, gT, params):
    """-> the loss and (dW1, db1, dW2, db2), in the order of the parameters"""
    W1, b1, W2, b2 = params
    h = nd.dnn_linear_forward(gX, W1, b1, "tanh")
    logits = nd.dnn_linear_forward(h, W2, b2)
    loss, dlogits = nd.dnn_cross_entropy(logits, gT, "mean", with_grad=True)
    dW2, dh, db2 = nd.dnn_linear_backward(h, dlogits, W2, bias=True)
    dW1, _, db1 = nd.dnn_linear_backward(gX, dh, W1, out=h, activation="tanh", bias=True, need_dx=False)
    return _value(loss), [dW1, db1, dW2, db2]


def train(samples: int = 512, features: int = 32, hidden: int = 64, classes: int = 4, steps: int = 40):
    """full-batch AdamW -> the first and the last loss"""
    X, labels = make_problem(samples, features, classes)
    gX, gT = nd.array(X).gpu(), nd.array(labels.astype(np.float32)).gpu()
    params = init_params(features, hidden, classes)
    opt = optim.AdamW(params, lr=LR, weight_decay=WEIGHT_DECAY)
    losses = []
    for _ in range(steps):
        loss, grads = gradients(gX, gT, params)
        losses.append(loss)
        opt.step(grads)
    return losses[0], losses[-1]


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    first, last = train(samples=samples, steps=steps)
    print("samples %d, %d AdamW steps: loss %.4f -> %.4f" % (samples, steps, first, last))
    assert last < 0.7 * first, "the loss did not fall"


if __name__ == "__main__":
    main()
