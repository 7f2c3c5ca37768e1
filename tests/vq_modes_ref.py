"""Host restatements for the quantizer-mode tests (float64 numpy): the noise contract of include/speechclip_hip.h and the train-mode arithmetic of
SimpleVectorQuantizer (my_vector_quantizer.py:75-79 masking, :124-131 modes; F.gumbel_softmax: gumbels = -log(Exponential(1)), y = softmax((x + gumbels) / tau),
hard: one-hot(arg-max y) in the forward, y in the backward; kwClip.py:909 keywords = subword_prob @ emb)."""
import numpy as np

MASK = (0, 2, 3)
MODES = {"soft": (False, False), "gumbel_hard": (True, True), "gumbel_soft": (True, False)}      # name -> (use_gumbel, hard)


def hash32(x):
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def hash_draw(seed, idx):
    """h = hash32(seed ^ hash32(idx + 0x9e3779b9)) for uint32 indices."""
    idx = np.asarray(idx, dtype=np.uint64)
    return hash32(np.uint64(int(seed) & 0xFFFFFFFF) ^ hash32((idx + 0x9E3779B9) & 0xFFFFFFFF))


def uniform(seed, idx):
    return ((hash_draw(seed, idx) >> 9).astype(np.float64) + 0.5) * 2.0 ** -23


def exponential(seed, idx):
    return -np.log(uniform(seed, idx))


def gumbel(seed, idx):
    return -np.log(exponential(seed, idx))


def gumbel_matrix(seed, R, V):
    return gumbel(seed, np.arange(R * V, dtype=np.uint64)).reshape(R, V)


def masked_logits(x, g, temp, mask=MASK):
    """z = (x + g) / T in float64 with the masked columns at -inf."""
    z = (np.asarray(x, np.float64) + (0.0 if g is None else g)) / float(temp)
    z[:, list(mask)] = -np.inf
    return z


def softmax(z):
    z = z - z.max(-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(-1, keepdims=True)


def mode_forward(x, emb, temp, use_gumbel, hard, seed=0, mask=MASK, f32_points=False):
    """(subword_prob, targets, keywords, y) of one train-mode setting, float64.
    f32_points: round where the reference class rounds -- it forms the noise, x + g and the division by T in fp32 (F.gumbel_softmax works on x.float(), and
    :130 divides an fp32 tensor) -- and continue in float64.  At T = 0.1 a logit (x + g) / T near 30 carries 2e-6 of fp32 rounding, which is 1e-6 of a
    probability near 1/2: a restatement that is to meet the reference's own numbers at 1e-6 has to round there too.  The GPU tests use the plain float64 form."""
    R, V = x.shape
    g = gumbel_matrix(seed, R, V) if use_gumbel else None
    if f32_points:
        f = np.float32
        s = np.asarray(x, f) if g is None else (np.asarray(x, f) + (-np.log(exponential(seed, np.arange(R * V, dtype=np.uint64)).astype(f).astype(np.float64))).astype(f).reshape(R, V))
        z = (s / f(temp)).astype(np.float64)
        z[:, list(mask)] = -np.inf
    else:
        z = masked_logits(x, g, temp, mask)
    y = softmax(z)
    targets = z.argmax(-1)                              # first index on ties, as torch.max
    prob = np.zeros_like(y)
    prob[np.arange(R), targets] = 1.0
    if not hard:
        prob = y
    return prob, targets, prob @ np.asarray(emb, np.float64), y


def mode_dx(y, dprob, temp):
    """d/dx of a loss with d loss / d subword_prob = dprob, through y = softmax((x + g) / T): y (dprob - sum y dprob) / T (masked columns: y = 0)."""
    return y * (dprob - (y * dprob).sum(-1, keepdims=True)) / float(temp)


def pack_f32(a):
    """fp32 array -> uint8 [4, n]: its four byte planes (the fixture's storage of dense arrays; lossless)."""
    return np.ascontiguousarray(np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint8).reshape(-1, 4).T)


def unpack_f32(planes, shape):
    return np.ascontiguousarray(planes.T).view(np.float32).reshape(shape)
