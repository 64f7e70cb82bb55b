"""One pre-norm attention block as a sequence classifier; every array is resident on the MI355X.

    h = X . W0                               (BATCH . TOKENS, HIDDEN): the token embedding through a matmul
    n, mean, invstd = dnn_layer_norm_forward(h, HIDDEN, gamma, beta)
    q, k, v = n . Wq, n . Wk, n . Wv         (BATCH, TOKENS, HEAD) each
    a, smax, ssum = dnn_attention_forward(q, k, v)
                                             fused: the (TOKENS, TOKENS) scores stay in the matrix core's accumulators
    pooled = POOL . a                        (BATCH, HEAD): the mean over the tokens, as a product with the averaging matrix
    logit = pooled . Wo                      (BATCH, CLASSES)
    loss, dlogit = dnn_cross_entropy(logit, labels, with_grad=True)
    backward: dWo and dpooled from dlogit; da = POOL^T . dpooled; dq, dk, dv = dnn_attention_backward(q, k, v, a, da, smax, ssum);
    the three projection gradients and dn = dq . Wq^T + dk . Wk^T + dv . Wv^T; dh, dgamma, dbeta = dnn_layer_norm_backward(h, dn,
    HIDDEN, gamma, mean, invstd); dW0 = X^T . dh.  Plain SGD, as the other examples.

The task: a sequence holds noise tokens and two copies of one of CLASSES marker tokens at random positions; the class is the marker.
`python examples/attention_classifier.py [samples] [epochs]` prints the loss per epoch; main() asserts that it falls.
tests/test_gpu_attention.py runs a small instance."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from numpower_amd.ndarray import NDArray as nd  # noqa: E402

TOKENS, EMBED, HIDDEN, HEAD, CLASSES = 12, 8, 16, 16, 4
BATCH = 8
LR = 0.2


def make_problem(samples: int, seed: int = 0):
    """-> X (samples, TOKENS, EMBED) float32, labels (samples,) int"""
    rng = np.random.default_rng(seed)
    markers = rng.standard_normal((CLASSES, EMBED)).astype(np.float32) * 2.0
    labels = rng.integers(0, CLASSES, samples)
    X = (0.5 * rng.standard_normal((samples, TOKENS, EMBED))).astype(np.float32)
    for s in range(samples):
        X[s, rng.choice(TOKENS, 2, replace=False)] += markers[labels[s]]
    return X, labels


def init_params(seed: int = 1):
    """-> [W0, gamma, beta, Wq, Wk, Wv, Wo]"""
    rng = np.random.default_rng(seed)
    w = lambda r, c: (rng.standard_normal((r, c)) / np.sqrt(r)).astype(np.float32)
    host = (w(EMBED, HIDDEN), np.ones(HIDDEN, np.float32), np.zeros(HIDDEN, np.float32), w(HIDDEN, HEAD), w(HIDDEN, HEAD), w(HIDDEN, HEAD),
            w(HEAD, CLASSES))
    return [nd.array(a).gpu() for a in host]


def pool_matrix(batch: int):
    """(batch, batch . TOKENS): row b averages the tokens of sample b"""
    P = np.zeros((batch, batch * TOKENS), np.float32)
    for b in range(batch):
        P[b, b * TOKENS:(b + 1) * TOKENS] = 1.0 / TOKENS
    return nd.array(P).gpu()


def forward(gX, params, pool):
    """gX: (batch . TOKENS, EMBED) -> everything the backward pass reads, the logits last"""
    W0, gamma, beta, Wq, Wk, Wv, Wo = params
    batch = gX.shape()[0] // TOKENS
    h = nd.matmul(gX, W0)
    n, mean, invstd = nd.dnn_layer_norm_forward(h, HIDDEN, gamma, beta)
    q, k, v = (nd.reshape(nd.matmul(n, W), [batch, TOKENS, HEAD]) for W in (Wq, Wk, Wv))
    a, smax, ssum = nd.dnn_attention_forward(q, k, v)
    pooled = nd.matmul(pool, nd.reshape(a, [batch * TOKENS, HEAD]))
    return h, n, mean, invstd, q, k, v, a, smax, ssum, pooled, nd.matmul(pooled, Wo)


def _value(loss):
    return float(loss) if isinstance(loss, (int, float, np.floating)) else float(np.asarray(loss.cpu().numpy()).reshape(-1)[0])


def train_gpu(X, labels, epochs: int, lr: float):
    """plain SGD over consecutive batches -> the parameters and the loss of every step"""
    params = init_params()
    pool = pool_matrix(BATCH)
    pool_t = nd.transpose(pool)
    losses = []
    for _ in range(epochs):
        for at in range(0, X.shape[0] - BATCH + 1, BATCH):
            gX = nd.array(X[at:at + BATCH].reshape(BATCH * TOKENS, EMBED)).gpu()
            gT = nd.array(labels[at:at + BATCH].astype(np.float32)).gpu()
            h, n, mean, invstd, q, k, v, a, smax, ssum, pooled, logit = forward(gX, params, pool)
            loss, dlogit = nd.dnn_cross_entropy(logit, gT, "mean", with_grad=True)
            losses.append(_value(loss))
            W0, gamma, beta, Wq, Wk, Wv, Wo = params
            dWo = nd.matmul(nd.transpose(pooled), dlogit)
            dpooled = nd.matmul(dlogit, nd.transpose(Wo))
            da = nd.reshape(nd.matmul(pool_t, dpooled), [BATCH, TOKENS, HEAD])
            dq, dk, dv = (nd.reshape(g, [BATCH * TOKENS, HEAD]) for g in nd.dnn_attention_backward(q, k, v, a, da, smax, ssum))
            nt = nd.transpose(n)
            dWq, dWk, dWv = nd.matmul(nt, dq), nd.matmul(nt, dk), nd.matmul(nt, dv)
            dn = nd.matmul(dq, nd.transpose(Wq)) + nd.matmul(dk, nd.transpose(Wk)) + nd.matmul(dv, nd.transpose(Wv))
            dh, dgamma, dbeta = nd.dnn_layer_norm_backward(h, dn, HIDDEN, gamma, mean, invstd)
            dW0 = nd.matmul(nd.transpose(gX), dh)
            params = [p - g * lr for p, g in zip(params, (dW0, dgamma, dbeta, dWq, dWk, dWv, dWo))]
    return params, losses


def predict(X, params):
    """the logits"""
    n = X.shape[0]
    return forward(nd.array(X.reshape(n * TOKENS, EMBED)).gpu(), params, pool_matrix(n))[-1].cpu().numpy().reshape(n, CLASSES)


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    X, labels = make_problem(samples)
    params, losses = train_gpu(X, labels, epochs, LR)
    per = samples // BATCH
    print("samples %d, epochs %d, batch %d" % (samples, epochs, BATCH))
    print("mean loss per epoch: " + " ".join("%.4f" % np.mean(losses[e * per:(e + 1) * per]) for e in range(epochs)))
    print("training accuracy %.3f" % float(np.mean(np.argmax(predict(X, params), axis=1) == labels)))
    assert np.mean(losses[-per:]) < 0.7 * np.mean(losses[:per]), "the loss did not fall"


if __name__ == "__main__":
    main()
