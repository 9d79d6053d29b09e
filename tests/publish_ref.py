"""A numpy restatement of the evaluator's layout function (include/az_nn.h, az_nn_publish_dev): what k_publish is held to
byte for byte.  State dict in as numpy float32, every destination array out as uint16 (bf16 bits) or float32, under the
twin's buffer names (fast_net.FastConnect4Net: block k is res{k + 2}_w / _b / _g / _beta).

bf16 is rounded to nearest-even by integer arithmetic on the float32 bits; the folded stem is computed in float32 in the
documented order - one multiply and one add per step, starting from +0 - and scattered into the fragment order.  The
keyword switches of `fold` build the WRONG variants the tests must tell apart from the right one."""
import numpy as np

ROWS, COLS, CELLS, EMB, CH, TAPS = 6, 7, 42, 32, 64, 9
ORBIT = np.array([4 * (cell // COLS) + min(cell % COLS, COLS - 1 - cell % COLS) for cell in range(CELLS)])

HEADS = (("p_norm", "policy_head.norm.weight"), ("p_gate_w", "policy_head.row_gate.weight"), ("p_fc_w", "policy_head.fc.weight"),
         ("p_fc_b", "policy_head.fc.bias"), ("p_out_w", "policy_head.out.weight"), ("d_pool_norm", "dual_head.pool_norm.weight"),
         ("d_pool_w", "dual_head.pool_fc.weight"), ("d_pool_b", "dual_head.pool_fc.bias"), ("d_norm", "dual_head.norm.weight"),
         ("d_fc_w", "dual_head.fc.weight"), ("d_fc_b", "dual_head.fc.bias"), ("d_out_norm", "dual_head.out_norm.weight"),
         ("d_val_w", "dual_head.value_out.weight"), ("d_val_b", "dual_head.value_out.bias"), ("d_aux_w", "dual_head.aux_out.weight"))
SCALARS = ("policy_head.row_gate.bias", "policy_head.out.bias", "dual_head.aux_out.bias")


def bf16_bits(x):
    """float32 -> the uint16 of its bfloat16, round to nearest, ties to even; a NaN stays a (quiet) NaN."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    rounded = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, rounded).astype(np.uint16)


def bf16_float(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_float(bf16_bits(x))


def n_blocks_of(sd):
    n = 0
    while "hidden.%d.conv.weight" % (n + 2) in sd:
        n += 1
    return n


def fold_tables(w, b, emb, pos_emb, swap_planes=False, bias_first=False, outside=False):
    """T [64][32] and pmap [48][68] in float32 from w [64][32][3][3] and b [64] AS GIVEN (the caller rounds them), the piece
    embeddings [2][32] and the position embeddings [24][32], in the documented order.  swap_planes: opponent first;
    bias_first: the running sum starts at b instead of ending with it; outside: a tap outside the board counts the
    nearest cell's position instead of nothing."""
    w = np.asarray(w, np.float32).reshape(CH, EMB, TAPS)
    emb, pos_emb, b = np.asarray(emb, np.float32), np.asarray(pos_emb, np.float32), np.asarray(b, np.float32)
    t = np.zeros((CH, 32), np.float32)
    for k in range(2 * TAPS):
        tap, plane = k // 2, (k % 2) ^ int(swap_planes)
        acc = np.zeros(CH, np.float32)
        for c in range(EMB):
            acc = acc + w[:, c, tap] * emb[plane, c]
        t[:, k] = acc
    acc = np.zeros((CELLS, CH), np.float32)
    if bias_first:
        acc = acc + b[None, :]
    ys, xs = np.arange(CELLS) // COLS, np.arange(CELLS) % COLS
    for tap in range(TAPS):
        yy, xx = ys + tap // 3 - 1, xs + tap % 3 - 1
        inside = (yy >= 0) & (yy < ROWS) & (xx >= 0) & (xx < COLS)
        orbit = ORBIT[np.clip(yy, 0, ROWS - 1) * COLS + np.clip(xx, 0, COLS - 1)]
        use = np.ones(CELLS, bool) if outside else inside
        for c in range(EMB):
            prod = pos_emb[orbit, c][:, None] * w[None, :, c, tap]
            acc = np.where(use[:, None], acc + prod, acc)
    if not bias_first:
        acc = acc + b[None, :]
    pmap = np.zeros((48, 68), np.float32)
    pmap[:CELLS, :CH] = acc
    return t, pmap


def split(t):
    """(hi, lo) bf16 bits of T: hi = bf16(T), lo = bf16(T - float(hi))."""
    hi = bf16_bits(t)
    return hi, bf16_bits(np.asarray(t, np.float32) - bf16_float(hi))


def fragments(hi, lo):
    """[2][4][64][8]: [part][channel tile i][lane][j] = part[32 (i / 2) + 8 (r / 4) + 4 (i % 2) + r % 4][8 (lane >> 4) + j]."""
    out = np.zeros((2, 4, 64, 8), np.uint16)
    for p, part in enumerate((hi, lo)):
        for i in range(4):
            for lane in range(64):
                r = lane & 15
                row = 32 * (i // 2) + 8 * (r // 4) + 4 * (i % 2) + r % 4
                out[p, i, lane] = part[row, 8 * (lane >> 4):8 * (lane >> 4) + 8]
    return out


def unfragment(frag):
    """The inverse of `fragments`: (hi, lo) bits as [64][32]."""
    parts = np.zeros((2, CH, 32), np.uint16)
    for p in range(2):
        for i in range(4):
            for lane in range(64):
                r = lane & 15
                row = 32 * (i // 2) + 8 * (r // 4) + 4 * (i % 2) + r % 4
                parts[p, row, 8 * (lane >> 4):8 * (lane >> 4) + 8] = frag[p, i, lane]
    return parts[0], parts[1]


def fold(sd, round_w=True, **variant):
    """(stem_frag uint16 [2][4][64][8], stem_pmap float32 [48][68]) of a state dict."""
    w, b = sd["hidden.0.weight"], sd["hidden.0.bias"]
    t, pmap = fold_tables(bf16_round(w) if round_w else w, bf16_round(b), sd["piece_emb.weight"], sd["pos_emb.weight"], **variant)
    return fragments(*split(t)), pmap


def ohwi(w):
    """OIHW float32 -> bf16 bits in OHWI memory order, [o][tap][c]."""
    w = np.asarray(w, np.float32)
    return bf16_bits(np.ascontiguousarray(w.reshape(w.shape[0], w.shape[1], TAPS).transpose(0, 2, 1)))


def layout(sd, folded=True):
    """Every destination of az_nn_publish_dev -> dict: bf16 arrays as uint16 in MEMORY order, stem_pmap and "scalars" (the
    three float32 biases) as float32."""
    sd = {k: np.ascontiguousarray(v, np.float32) for k, v in sd.items() if k != "orbit_map"}
    out = {"emb_own": bf16_bits(sd["piece_emb.weight"][0]), "emb_opp": bf16_bits(sd["piece_emb.weight"][1]),
           "pos": bf16_bits(sd["pos_emb.weight"][ORBIT]), "stem_w": ohwi(sd["hidden.0.weight"]), "stem_b": bf16_bits(sd["hidden.0.bias"])}
    n = n_blocks_of(sd)
    for k in range(n):
        p = "hidden.%d." % (k + 2)
        out["res%d_w" % (k + 2)] = ohwi(sd[p + "conv.weight"])
        out["res%d_b" % (k + 2)] = bf16_bits(sd[p + "conv.bias"])
        out["res%d_g" % (k + 2)] = bf16_bits(sd[p + "norm.weight"])
        out["res%d_beta" % (k + 2)] = bf16_bits(sd[p + "norm.bias"])
    a = "hidden.%d.attn." % (n + 2)
    out["pre_w"] = bf16_bits(sd[a + "prenorm.weight"])
    out["qkvg_w"] = bf16_bits(np.concatenate([sd[a + "qkv_proj.weight"], sd[a + "gate_proj.weight"]], 0))
    out["o_w"] = bf16_bits(sd[a + "o_proj.weight"])
    out["qn_w"] = bf16_bits(sd[a + "q_norm.weight"])
    out["kn_w"] = bf16_bits(sd[a + "k_norm.weight"])
    for name, key in HEADS:
        out[name] = bf16_bits(sd[key].reshape(-1) if sd[key].shape[0] == 1 else sd[key])
    if folded:
        out["stem_frag"], out["stem_pmap"] = fold(sd)
    out["scalars"] = np.array([sd[k].reshape(-1)[0] for k in SCALARS], np.float32)
    return out


def fold_float64(sd):
    """T [64][18] and pmap [42][64] in float64 on the bf16-rounded W and bias, with the sums of absolute products S, S'
    (|b| inside S') that the error bounds are stated in."""
    w = bf16_round(sd["hidden.0.weight"]).astype(np.float64).reshape(CH, EMB, TAPS)
    b = bf16_round(sd["hidden.0.bias"]).astype(np.float64)
    emb, pos_emb = np.asarray(sd["piece_emb.weight"], np.float64), np.asarray(sd["pos_emb.weight"], np.float64)
    t = np.einsum("oct,pc->otp", w, emb).reshape(CH, 18)
    s = np.einsum("oct,pc->otp", np.abs(w), np.abs(emb)).reshape(CH, 18)
    pmap, sp = np.zeros((CELLS, CH)), np.zeros((CELLS, CH))
    for cell in range(CELLS):
        for tap in range(TAPS):
            yy, xx = cell // COLS + tap // 3 - 1, cell % COLS + tap % 3 - 1
            if 0 <= yy < ROWS and 0 <= xx < COLS:
                p = pos_emb[ORBIT[yy * COLS + xx]]
                pmap[cell] += w[:, :, tap] @ p
                sp[cell] += np.abs(w[:, :, tap]) @ np.abs(p)
    return t, s, pmap + b[None, :], sp + np.abs(b)[None, :]
