"""A two-layer convolutional classifier trained with the device conv layers, every array resident on the MI355X.

    h = relu(conv3x3(x, W1) + b1)            dnn_conv2d_forward(..., bias=, activation='relu'): bias and relu in the kernel's epilogue
    p = sigmoid(conv(h, W2) + b2)            a window as large as h: one output pixel per class, (N, classes, 1, 1)
    loss = sum((p - Y)^2) / (2 N)
    backward: dnn_conv2d_backward(..., out=, activation=, bias=True) gives (dW, dX, db) from the layer's OUTPUT; dX of the
    second layer is the gradient of the first one's output.

Synthetic data: class c is a bright square in quadrant c of a noisy 12 x 12 image.  `python examples/conv_classifier.py [samples]
[steps]` prints the loss curve; main() asserts that the loss falls.  tests/test_gpu_dnn_act.py runs a small instance."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from numpower_amd.ndarray import NDArray as nd  # noqa: E402

SIDE, CLASSES, HIDDEN = 12, 4, 8


def make_problem(samples: int, seed: int = 1):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, CLASSES, samples)
    X = (0.3 * rng.standard_normal((samples, 1, SIDE, SIDE))).astype(np.float32)
    half = SIDE // 2
    for n, c in enumerate(labels):
        r, q = (c // 2) * half, (c % 2) * half
        X[n, 0, r + 1:r + half - 1, q + 1:q + half - 1] += 1.0
    Y = np.zeros((samples, CLASSES, 1, 1), np.float32)
    Y[np.arange(samples), labels] = 1.0
    return X, Y, labels


def init_params(seed: int = 2):
    rng = np.random.default_rng(seed)
    W1 = (0.3 * rng.standard_normal((HIDDEN, 1, 3, 3))).astype(np.float32)
    W2 = (0.05 * rng.standard_normal((CLASSES, HIDDEN, SIDE, SIDE))).astype(np.float32)
    return [nd.array(a).gpu() for a in (W1, np.zeros(HIDDEN, np.float32), W2, np.zeros(CLASSES, np.float32))]


def forward(gX, params):
    W1, b1, W2, b2 = params
    h = nd.dnn_conv2d_forward(gX, W1, padding="same", bias=b1, activation="relu")
    return h, nd.dnn_conv2d_forward(h, W2, bias=b2, activation="sigmoid")


def train_gpu(X, Y, steps: int, lr: float):
    n = X.shape[0]
    gX, gY = nd.array(X).gpu(), nd.array(Y).gpu()
    params = init_params()
    losses = []
    for _ in range(steps):
        h, p = forward(gX, params)
        diff = p - gY
        losses.append(float(nd.sum(diff * diff)) / (2 * n))
        dW2, dh, db2 = nd.dnn_conv2d_backward(h, diff * (1.0 / n), params[2], out=p, activation="sigmoid", bias=True)
        dW1, _, db1 = nd.dnn_conv2d_backward(gX, dh, params[0], padding="same", out=h, activation="relu", bias=True)
        params = [a - g * lr for a, g in zip(params, (dW1, db1, dW2, db2))]
    _, p = forward(gX, params)
    return params, losses, p.cpu().numpy().reshape(n, CLASSES)


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    X, Y, labels = make_problem(samples)
    _, losses, p = train_gpu(X, Y, steps, 0.1)
    print("samples %d, steps %d" % (samples, steps))
    print("loss: " + " ".join("%.4f" % v for v in losses))
    print("training accuracy %.3f" % float(np.mean(np.argmax(p, axis=1) == labels)))
    assert losses[-1] < 0.5 * losses[0], "the loss did not fall"


if __name__ == "__main__":
    main()
