"""The classifier of examples/conv_bn_classifier.py with a group normalization in place of the batch normalization, trained at a
batch size of 2: the case batch normalization serves badly, since its statistics would run over two samples.  Every array is
resident on the MI355X.

    c = conv3x3(x, W1)                       (2, HIDDEN, 12, 12), padding 'same', no bias (beta takes its place), no fused activation
    a, mean, invstd = dnn_group_norm_forward(c, GROUPS, gamma, beta)
                                             per (sample, group) over (HIDDEN / GROUPS, 12, 12): fp64 shifted sums, a row of 576
                                             values in the registers of one wave; nothing depends on the batch
    h = maximum(a, 0)                        relu from the elementwise ops
    q = maxpool2x2/2(h)                      (2, HIDDEN, 6, 6)
    z = conv3x3(q, W2) + b2                  (2, CLASSES, 6, 6), padding 'same'
    logit = avgpool(z), window = image       (2, CLASSES)
    loss, dlogit = dnn_cross_entropy(logit, labels, with_grad=True)
    backward: as in conv_bn_classifier.py down to da; dc, dgamma, dbeta = dnn_group_norm_backward(c, da, GROUPS, gamma, mean,
    invstd); dW1 from dc.

There are no running statistics: inference is the same call.  `python examples/conv_gn_classifier.py [samples] [epochs]` prints the
loss per epoch; main() asserts that it falls.  tests/test_gpu_groupnorm.py runs a small instance."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from examples.conv_bn_classifier import CLASSES, HIDDEN, POOLED, make_problem  # noqa: E402,F401
from numpower_amd.ndarray import NDArray as nd  # noqa: E402

GROUPS = 2
BATCH = 2


def init_params(seed: int = 2):
    """-> [W1, gamma, beta, W2, b2]"""
    rng = np.random.default_rng(seed)
    W1 = (0.3 * rng.standard_normal((HIDDEN, 1, 3, 3))).astype(np.float32)
    W2 = (0.1 * rng.standard_normal((CLASSES, HIDDEN, 3, 3))).astype(np.float32)
    return [nd.array(a).gpu() for a in (W1, np.ones(HIDDEN, np.float32), np.zeros(HIDDEN, np.float32), W2, np.zeros(CLASSES, np.float32))]


def forward(gX, params):
    W1, gamma, beta, W2, b2 = params
    c = nd.dnn_conv2d_forward(gX, W1, padding="same")
    a, mean, invstd = nd.dnn_group_norm_forward(c, GROUPS, gamma, beta)
    h = nd.maximum(a, 0.0)
    q = nd.dnn_pool2d_forward(h, 2)
    z = nd.dnn_conv2d_forward(q, W2, padding="same", bias=b2)
    return c, mean, invstd, h, q, z, nd.dnn_pool2d_forward(z, (POOLED, POOLED), mode="avg")


def _value(loss):
    return float(loss) if isinstance(loss, (int, float, np.floating)) else float(np.asarray(loss.cpu().numpy()).reshape(-1)[0])


def train_gpu(X, labels, epochs: int, lr: float):
    """plain SGD over consecutive pairs of samples -> the parameters and the loss of every step"""
    params = init_params()
    losses = []
    for _ in range(epochs):
        for at in range(0, X.shape[0] - BATCH + 1, BATCH):
            gX, gT = nd.array(X[at:at + BATCH]).gpu(), nd.array(labels[at:at + BATCH].astype(np.float32)).gpu()
            c, mean, invstd, h, q, z, logit = forward(gX, params)
            loss, dlogit = nd.dnn_cross_entropy(nd.reshape(logit, [BATCH, CLASSES]), gT, "mean", with_grad=True)
            losses.append(_value(loss))
            dz = nd.dnn_pool2d_backward(z, nd.reshape(dlogit, [BATCH, CLASSES, 1, 1]), (POOLED, POOLED), mode="avg")
            dW2, dq, db2 = nd.dnn_conv2d_backward(q, dz, params[3], padding="same", bias=True)
            dh = nd.dnn_pool2d_backward(h, dq, 2)
            da = dh * nd.greater(h, 0.0)
            dc, dgamma, dbeta = nd.dnn_group_norm_backward(c, da, GROUPS, params[1], mean, invstd)
            dW1, _ = nd.dnn_conv2d_backward(gX, dc, params[0], padding="same")
            params = [p - g * lr for p, g in zip(params, (dW1, dgamma, dbeta, dW2, db2))]
    return params, losses


def predict(X, params):
    """the logits; group normalization is the same call in training and inference"""
    return forward(nd.array(X).gpu(), params)[6].cpu().numpy().reshape(X.shape[0], CLASSES)


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    X, labels = make_problem(samples)
    params, losses = train_gpu(X, labels, epochs, 0.05)
    per = samples // BATCH
    print("samples %d, epochs %d, batch %d" % (samples, epochs, BATCH))
    print("mean loss per epoch: " + " ".join("%.4f" % np.mean(losses[e * per:(e + 1) * per]) for e in range(epochs)))
    print("training accuracy %.3f" % float(np.mean(np.argmax(predict(X, params), axis=1) == labels)))
    assert np.mean(losses[-per:]) < 0.5 * np.mean(losses[:per]), "the loss did not fall"


if __name__ == "__main__":
    main()
