"""The CNN of examples/conv_pool_classifier.py trained as a classifier: a softmax over the class logits and the cross-entropy loss,
every array resident on the MI355X.

    h = relu(conv3x3(x, W1) + b1)            (N, HIDDEN, 12, 12), padding 'same'
    q = maxpool2x2/2(h)                      (N, HIDDEN, 6, 6)
    z = conv3x3(q, W2) + b2                  (N, CLASSES, 6, 6), padding 'same'
    logit = avgpool(z), window = image       (N, CLASSES, 1, 1), seen as (N, CLASSES)
    loss, dlogit = dnn_cross_entropy(logit, labels, with_grad=True)
                                             the mean of log(sum exp(l - max)) - (l - max)[label], and (softmax(logit) - onehot) / N
                                             from the same launch: the logits are read once, and a saturated logit costs its gap,
                                             not an infinity
    backward: dlogit goes back through the average pool, the second convolution, the max pool and the first convolution exactly
    as the squared-error gradient does in conv_pool_classifier.py.

The labels are class indices stored as fp32, (N,).  Synthetic data as in conv_pool_classifier.py: the class is a TEXTURE at a random
phase under noise.  `python examples/conv_softmax_classifier.py [samples] [steps]` prints the loss curve; main() asserts that the
loss falls.  tests/test_gpu_softmax.py runs a small instance."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from numpower_amd.ndarray import NDArray as nd  # noqa: E402

SIDE, CLASSES, HIDDEN = 12, 4, 8
POOLED = SIDE // 2


def make_problem(samples: int, seed: int = 1):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, CLASSES, samples)
    r, c = np.mgrid[0:SIDE, 0:SIDE]
    X = (0.3 * rng.standard_normal((samples, 1, SIDE, SIDE))).astype(np.float32)
    for n, k in enumerate(labels):
        a, b = rng.integers(0, 2, 2)
        pattern = ((r + a) % 2, (c + b) % 2, (r + c + a) % 2, np.ones_like(r))[k]
        X[n, 0] += (2.0 * pattern - 1.0 if k < 3 else pattern).astype(np.float32)
    return X, labels


def init_params(seed: int = 2):
    rng = np.random.default_rng(seed)
    W1 = (0.3 * rng.standard_normal((HIDDEN, 1, 3, 3))).astype(np.float32)
    W2 = (0.1 * rng.standard_normal((CLASSES, HIDDEN, 3, 3))).astype(np.float32)
    return [nd.array(a).gpu() for a in (W1, np.zeros(HIDDEN, np.float32), W2, np.zeros(CLASSES, np.float32))]


def forward(gX, params):
    W1, b1, W2, b2 = params
    h = nd.dnn_conv2d_forward(gX, W1, padding="same", bias=b1, activation="relu")
    q = nd.dnn_pool2d_forward(h, 2)
    z = nd.dnn_conv2d_forward(q, W2, padding="same", bias=b2)
    return h, q, z, nd.dnn_pool2d_forward(z, (POOLED, POOLED), mode="avg")


def train_gpu(X, labels, steps: int, lr: float):
    n = X.shape[0]
    gX, gT = nd.array(X).gpu(), nd.array(labels.astype(np.float32)).gpu()
    params = init_params()
    losses = []
    for _ in range(steps):
        h, q, z, logit = forward(gX, params)
        loss, dlogit = nd.dnn_cross_entropy(nd.reshape(logit, [n, CLASSES]), gT, "mean", with_grad=True)
        losses.append(loss)
        dz = nd.dnn_pool2d_backward(z, nd.reshape(dlogit, [n, CLASSES, 1, 1]), (POOLED, POOLED), mode="avg")
        dW2, dq, db2 = nd.dnn_conv2d_backward(q, dz, params[2], padding="same", bias=True)
        dh = nd.dnn_pool2d_backward(h, dq, 2)
        dW1, _, db1 = nd.dnn_conv2d_backward(gX, dh, params[0], padding="same", out=h, activation="relu", bias=True)
        params = [a - g * lr for a, g in zip(params, (dW1, db1, dW2, db2))]
    logit = forward(gX, params)[3]
    return params, losses, logit.cpu().numpy().reshape(n, CLASSES)


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    X, labels = make_problem(samples)
    _, losses, logit = train_gpu(X, labels, steps, 0.1)
    print("samples %d, steps %d" % (samples, steps))
    print("loss: " + " ".join("%.4f" % v for v in losses))
    print("training accuracy %.3f" % float(np.mean(np.argmax(logit, axis=1) == labels)))
    assert losses[-1] < 0.5 * losses[0], "the loss did not fall"


if __name__ == "__main__":
    main()
