"""The shadow-8 FILTER's bias fold, restated in numpy (no GPU): C_q and the per-query guard term.

The FILTER's MFMAs take the f16 operand m_d = 1152 + s_d (s_d the int8 value of the shadow, the stored byte s_d + 128
under the high byte 0x64) and the f16 query q^_d.  sum_d q^_d m_d = C_q + sum_d q^_d s_d with C_q = 1152 sum_d q^_d, so
every accumulator starts at -C_q rounded once to fp32.  Consecutive MFMAs of an accumulator are chained in k order, 16
elements each; inside one instruction the 16 products (exact in fp32: 11 x 11 significant bits) and the accumulator
are added in an order nobody documents.

Guard term (before the row scale), 2^-23 per add as the constant of the plain sum (gamma = (dpad + 64) 2^-23):
  * the value P_k = -C_q + 1152 sum_{d < 16 k} q^_d that enters instruction k can be part of the result of each of
    its 16 adds, whatever their order: 16 |P_k| 2^-23, summed over the instructions;
  * each of the instruction's 16 products, at most 1279 |q^_d|, likewise: 16 * 1279 * sum_d |q^_d| * 2^-23 in all;
  * the rounding of C_q to fp32: |C_q - fl(C_q)|;
  * all of it times 1 + 2^-10 for the second-order terms (at most dpad + 64 roundings of 2^-23 each on the sums above).
What the scores themselves (sum q^_d s_d) put into the partial sums is the plain sum's term and stays in the old E.
E grows by the term times the largest row scale of the shadow (scale_r = max_d |x_rd| / 127 in fp32)."""
import numpy as np

OFFSET = 1152.0   # 1024 (the f16 0x6400) + 128 (the shadow's byte offset)
OPERAND_MAX = 1279.0


def c_q(qh):
    """C_q in fp64 and the fp32 start value -C_q of the accumulators; qh: dequantised f16 queries [B][dpad], float64."""
    c = OFFSET * qh.sum(axis=1)
    return c, (-c).astype(np.float32)


def bias_term(qh):
    """The per-query term before the row scale; qh [B][dpad] float64, dpad a multiple of 16."""
    B, dpad = qh.shape
    assert dpad % 16 == 0
    c, start = c_q(qh)
    blocks = qh.reshape(B, dpad // 16, 16).sum(axis=2)
    # P_k for k = 0 .. S-1: the start value plus the blocks before k
    before = np.concatenate([np.zeros((B, 1)), np.cumsum(blocks, axis=1)[:, :-1]], axis=1)
    chain = np.abs(start.astype(np.float64)[:, None] + OFFSET * before).sum(axis=1)
    inst = OPERAND_MAX * np.abs(qh).sum(axis=1)
    return (2.0 ** -23 * 16.0 * (chain + inst) + np.abs(c + start.astype(np.float64))) * (1.0 + 2.0 ** -10)


def fold_fits(dim, B):
    """The FILTER folds where the row of -C_q fits in LDS behind the query tile (dpad / 16 KiB per 32-query block, two
    blocks for more than 32 queries if they fit) and the threshold row: everywhere but 1280 dims at 64 queries."""
    dpad = (dim + 63) // 64 * 64
    tile = lambda qb: dpad // 16 * qb * 1024
    qb = 2 if B > 32 and tile(2) <= 160 * 1024 else 1
    return tile(qb) + 2 * qb * 128 <= 160 * 1024


def guard_e8(qp, dim, max_norm, u_x8, max_scale, folded=True):
    """E_q of a shadow-8 scan, float64: the plain shadow-8 bound (guard_e with acc_gamma8 and u_x8) plus, where the FILTER
    folds (fold_fits), the bias term times the largest row scale.  qp: processed fp32 queries [B][dim].  Returns (E, old
    E, f16 queries)."""
    dpad = (dim + 63) // 64 * 64
    qh = np.zeros((len(qp), dpad))
    qh[:, :dim] = qp.astype(np.float16).astype(np.float64)
    q64 = np.zeros((len(qp), dpad))
    q64[:, :dim] = qp.astype(np.float64)
    dq = np.sqrt(((q64 - qh) ** 2).sum(axis=1))
    nq = np.sqrt((qh * qh).sum(axis=1))
    gamma = ((dpad + 64) * 2.0 ** -23 + 2.0 ** -23) * (1.0 + u_x8)
    old = max_norm * (dq * (1 + 1e-6) + (gamma + u_x8) * nq) + 1e-9
    return old + (bias_term(qh) * float(max_scale) if folded else 0.0), old, qh


def max_scale(stored_f32):
    """The largest row scale of the shadow, as k_shadow8 computes it: fp32 max|x| / 127 per row."""
    return float((np.abs(stored_f32).max(axis=1).astype(np.float32) / np.float32(127.0)).max())


def chained_fp32(qh, m, start, order):
    """fp32 emulation of one accumulator per (query, row): start, then 16-wide instructions chained in k order; inside
    an instruction the accumulator and the 16 exact products are added in `order` (forward: accumulator first, then
    the products in d order; reverse: products last to first, accumulator last; pairwise: a tree over the 17 terms).
    qh [B][dpad] float64 (f16 values), m [n][dpad] float64 (operands), start [B] float32.  Returns [B][n] float32."""
    B, dpad = qh.shape
    acc = np.repeat(start.astype(np.float32)[:, None], len(m), axis=1)
    q32, m32 = qh.astype(np.float32), m.astype(np.float32)
    for k in range(dpad // 16):
        prod = q32[:, None, 16 * k:16 * k + 16] * m32[None, :, 16 * k:16 * k + 16]  # exact in fp32
        terms = [acc] + [prod[:, :, j] for j in range(16)]
        if order == "forward":
            for t in terms[1:]:
                acc = (acc + t).astype(np.float32)
        elif order == "reverse":
            s = terms[16]
            for t in terms[15:0:-1]:
                s = (s + t).astype(np.float32)
            acc = (s + terms[0]).astype(np.float32)
        elif order == "pairwise":
            while len(terms) > 1:
                nxt = [(terms[i] + terms[i + 1]).astype(np.float32) for i in range(0, len(terms) - 1, 2)]
                if len(terms) % 2:
                    nxt.append(terms[-1])
                terms = nxt
            acc = terms[0]
        else:
            raise KeyError(order)
    return acc
