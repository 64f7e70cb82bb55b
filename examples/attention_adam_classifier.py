"""The attention classifier of attention_classifier.py trained with AdamW and gradient-norm clipping; every array is resident on the
MI355X and the whole update is three launches whatever the number of parameters.

    the model, the task and the forward pass are attention_classifier.py's, imported
    grads = gradients(...)                   the backward pass of that file, returning the seven gradients
    opt = optim.AdamW(params, lr=LR, weight_decay=WEIGHT_DECAY)
    opt.step(grads, max_norm=1.0)            dnn_grad_norm over the seven gradients (two launches: partials, fold), then ONE
                                             dnn_adam_step that reads the clip coefficient on the device: no host read, no
                                             allocation per parameter; the parameters are updated in place

`python examples/attention_adam_classifier.py [samples] [epochs]` prints the loss per epoch; main() asserts that it falls.
tests/test_gpu_optim.py runs a small instance."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from attention_classifier import (BATCH, CLASSES, EMBED, HEAD, HIDDEN, TOKENS, _value, forward, init_params, make_problem,  # noqa: E402,F401
                                  pool_matrix, predict)
from numpower_amd import optim  # noqa: E402
from numpower_amd.ndarray import NDArray as nd  # noqa: E402

LR = 0.02
WEIGHT_DECAY = 0.01
MAX_NORM = 1.0


def gradients(gX, gT, params, pool, pool_t):
    """-> the loss and (dW0, dgamma, dbeta, dWq, dWk, dWv, dWo), in the order of the parameters"""
    W0, gamma, beta, Wq, Wk, Wv, Wo = params
    h, n, mean, invstd, q, k, v, a, smax, ssum, pooled, logit = forward(gX, params, pool)
    loss, dlogit = nd.dnn_cross_entropy(logit, gT, "mean", with_grad=True)
    dWo = nd.matmul(nd.transpose(pooled), dlogit)
    dpooled = nd.matmul(dlogit, nd.transpose(Wo))
    da = nd.reshape(nd.matmul(pool_t, dpooled), [BATCH, TOKENS, HEAD])
    dq, dk, dv = (nd.reshape(g, [BATCH * TOKENS, HEAD]) for g in nd.dnn_attention_backward(q, k, v, a, da, smax, ssum))
    nt = nd.transpose(n)
    dWq, dWk, dWv = nd.matmul(nt, dq), nd.matmul(nt, dk), nd.matmul(nt, dv)
    dn = nd.matmul(dq, nd.transpose(Wq)) + nd.matmul(dk, nd.transpose(Wk)) + nd.matmul(dv, nd.transpose(Wv))
    dh, dgamma, dbeta = nd.dnn_layer_norm_backward(h, dn, HIDDEN, gamma, mean, invstd)
    dW0 = nd.matmul(nd.transpose(gX), dh)
    return _value(loss), [dW0, dgamma, dbeta, dWq, dWk, dWv, dWo]


def train_gpu(X, labels, epochs: int, lr: float = LR, weight_decay: float = WEIGHT_DECAY, max_norm: float = MAX_NORM):
    """AdamW with clipping over consecutive batches -> the parameters, the loss of every step and the optimizer"""
    params = init_params()
    opt = optim.AdamW(params, lr=lr, weight_decay=weight_decay)
    pool = pool_matrix(BATCH)
    pool_t = nd.transpose(pool)
    losses = []
    for _ in range(epochs):
        for at in range(0, X.shape[0] - BATCH + 1, BATCH):
            gX = nd.array(X[at:at + BATCH].reshape(BATCH * TOKENS, EMBED)).gpu()
            gT = nd.array(labels[at:at + BATCH].astype(np.float32)).gpu()
            loss, grads = gradients(gX, gT, params, pool, pool_t)
            losses.append(loss)
            opt.step(grads, max_norm=max_norm)
    return params, losses, opt


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    X, labels = make_problem(samples)
    params, losses, opt = train_gpu(X, labels, epochs)
    per = samples // BATCH
    print("samples %d, epochs %d, batch %d, %d AdamW steps" % (samples, epochs, BATCH, opt.steps))
    print("mean loss per epoch: " + " ".join("%.4f" % np.mean(losses[e * per:(e + 1) * per]) for e in range(epochs)))
    print("last gradient norm and clip coefficient: %.4f %.4f" % tuple(opt.last_norm.cpu().numpy()))
    print("training accuracy %.3f" % float(np.mean(np.argmax(predict(X, params), axis=1) == labels)))
    assert np.mean(losses[-per:]) < 0.7 * np.mean(losses[:per]), "the loss did not fall"


if __name__ == "__main__":
    main()
