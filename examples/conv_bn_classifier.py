"""The classifier of examples/conv_softmax_classifier.py with a batch normalization between the first convolution and its relu,
every array resident on the MI355X.

    c = conv3x3(x, W1)                       (N, HIDDEN, 12, 12), padding 'same', no bias (beta takes its place), no fused activation
    a, mean, invstd = dnn_batch_norm_forward(c, gamma, beta, running_mean, running_var)
                                             per channel over (N, 12, 12): fp64 shifted sums, one launch for channels this small;
                                             the running statistics are updated in place
    h = maximum(a, 0)                        relu from the elementwise ops
    q = maxpool2x2/2(h)                      (N, HIDDEN, 6, 6)
    z = conv3x3(q, W2) + b2                  (N, CLASSES, 6, 6), padding 'same'
    logit = avgpool(z), window = image       (N, CLASSES)
    loss, dlogit = dnn_cross_entropy(logit, labels, with_grad=True)
    backward: as in conv_softmax_classifier.py down to dh; da = dh . (h > 0); dc, dgamma, dbeta = dnn_batch_norm_backward(c, da,
    gamma, mean, invstd); dW1 from dc.

Inference uses the running statistics: predict() normalizes with training=False.  `python examples/conv_bn_classifier.py [samples]
[steps]` prints the loss curve; main() asserts that the loss falls.  tests/test_gpu_batchnorm.py runs a small instance."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from numpower_amd.ndarray import NDArray as nd  # noqa: E402

SIDE, CLASSES, HIDDEN = 12, 4, 8
POOLED = SIDE // 2
MOMENTUM = 0.1


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
    """-> [W1, gamma, beta, W2, b2], [running_mean, running_var]"""
    rng = np.random.default_rng(seed)
    W1 = (0.3 * rng.standard_normal((HIDDEN, 1, 3, 3))).astype(np.float32)
    W2 = (0.1 * rng.standard_normal((CLASSES, HIDDEN, 3, 3))).astype(np.float32)
    params = [nd.array(a).gpu() for a in (W1, np.ones(HIDDEN, np.float32), np.zeros(HIDDEN, np.float32), W2, np.zeros(CLASSES, np.float32))]
    running = [nd.array(a).gpu() for a in (np.zeros(HIDDEN, np.float32), np.ones(HIDDEN, np.float32))]
    return params, running


def forward(gX, params, running, training=True):
    W1, gamma, beta, W2, b2 = params
    c = nd.dnn_conv2d_forward(gX, W1, padding="same")
    if training:
        a, mean, invstd = nd.dnn_batch_norm_forward(c, gamma, beta, running[0], running[1], True, MOMENTUM)
    else:
        a, mean, invstd = nd.dnn_batch_norm_forward(c, gamma, beta, running[0], running[1], False), None, None
    h = nd.maximum(a, 0.0)
    q = nd.dnn_pool2d_forward(h, 2)
    z = nd.dnn_conv2d_forward(q, W2, padding="same", bias=b2)
    return c, mean, invstd, h, q, z, nd.dnn_pool2d_forward(z, (POOLED, POOLED), mode="avg")


def train_gpu(X, labels, steps: int, lr: float):
    n = X.shape[0]
    gX, gT = nd.array(X).gpu(), nd.array(labels.astype(np.float32)).gpu()
    params, running = init_params()
    losses = []
    for _ in range(steps):
        c, mean, invstd, h, q, z, logit = forward(gX, params, running)
        loss, dlogit = nd.dnn_cross_entropy(nd.reshape(logit, [n, CLASSES]), gT, "mean", with_grad=True)
        losses.append(loss)
        dz = nd.dnn_pool2d_backward(z, nd.reshape(dlogit, [n, CLASSES, 1, 1]), (POOLED, POOLED), mode="avg")
        dW2, dq, db2 = nd.dnn_conv2d_backward(q, dz, params[3], padding="same", bias=True)
        dh = nd.dnn_pool2d_backward(h, dq, 2)
        da = dh * nd.greater(h, 0.0)
        dc, dgamma, dbeta = nd.dnn_batch_norm_backward(c, da, params[1], mean, invstd)
        dW1, _ = nd.dnn_conv2d_backward(gX, dc, params[0], padding="same")
        params = [p - g * lr for p, g in zip(params, (dW1, dgamma, dbeta, dW2, db2))]
    return params, running, losses


def predict(X, params, running):
    """the logits under inference-mode normalization (the running statistics)"""
    logit = forward(nd.array(X).gpu(), params, running, training=False)[6]
    return logit.cpu().numpy().reshape(X.shape[0], CLASSES)


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    X, labels = make_problem(samples)
    params, running, losses = train_gpu(X, labels, steps, 0.1)
    print("samples %d, steps %d" % (samples, steps))
    print("loss: " + " ".join("%.4f" % v for v in losses))
    print("training accuracy under the running statistics %.3f" % float(np.mean(np.argmax(predict(X, params, running), axis=1) == labels)))
    assert losses[-1] < 0.5 * losses[0], "the loss did not fall"


if __name__ == "__main__":
    main()
