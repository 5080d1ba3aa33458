"""BigBird's block-sparse attention pattern as per-head, per-query-block lists of key blocks (ops/attention.py
``block_lists``): what transformers' ``BigBirdPegasusBlockSparseAttention`` attends to, entry for entry.

With ``n = ceil(S / block)`` blocks, query blocks 0 and n - 1 (the global rows) list every block; block 1 lists
``[0, 1, 2, n - 1] + rand[0]``, block n - 2 ``[0, n - 3, n - 2, n - 1] + rand[n - 3]`` and block i in 2 .. n - 3
``[0, i - 1, i, i + 1] + rand[i - 1] + [n - 1]``: 2 global blocks, 3 sliding blocks and ``num_random_blocks`` random
ones.  A block that stands twice in a list counts twice in the softmax — that is what transformers computes (it
concatenates the gathered key blocks and takes one softmax over them), and it happens:

* in eval mode its "random" blocks are all block 0, which every sliding row lists already;
* at the padded lengths 1024 / 3072 / 4096 it uses an old plan drawn for ``max_position_embeddings`` and cut to n - 2
  rows, whose draws do not exclude a row's own window.

``rand`` follows transformers' rule, quirks included, decided on the padded length ``n * block``; the draws are those
of ``np.random.seed(seed)`` followed by its ``np.random.permutation`` calls, made here on a private
``np.random.RandomState(seed)`` so that numpy's global state is left alone.  ``seed`` is the encoder layer's index.
"""
from __future__ import annotations

import numpy as np

from ..ops.attention import BlockLists, block_lists

_OLD_PLAN_LENGTHS = (1024, 3072, 4096)  # "old plans used in paper" (modeling_bigbird_pegasus.py)


def full_attention_rule(seq_len: int, block_size: int, num_random_blocks: int) -> bool:
    """transformers' rule for falling back to full attention: the sequence is no longer than the 2 global, 3 sliding
    and 2 x ``num_random_blocks`` random blocks a row could attend to."""
    return seq_len <= (5 + 2 * num_random_blocks) * block_size


def _rand_plan(from_seq_length: int, block: int, r: int) -> tuple[list, list]:
    """``_get_rand_attn_plan``: where the random blocks are drawn from, as (end positions, blocks per stretch)."""
    n = from_seq_length // block
    if 2 * r + 5 < n:
        return [(2 * r + 5) * block, from_seq_length], [r, 0]
    if r + 5 < n:
        return [(r + 5) * block, from_seq_length], [r // 2, r - r // 2]
    return [from_seq_length], [r]


def _old_plan(rs, seq_length: int, block: int, r: int, training: bool, last_idx: int) -> np.ndarray:
    """``_bigbird_block_rand_mask``: one head's ``[seq_length / block - 2, r]`` random blocks, the plan of the paper."""
    nb = seq_length // block
    rand = np.zeros((nb - 2, r), dtype=np.int32)
    if not training:
        return rand
    middle = np.arange(1, nb - 1, dtype=np.int32)
    last = nb - 1
    if last_idx > 2 * block:
        last = last_idx // block - 1
    for i in range(1, nb - 1):
        start, end = i - 2, i
        if i == 1:
            rand[i - 1, :] = rs.permutation(middle[2:last])[:r]
        elif i == 2:
            rand[i - 1, :] = rs.permutation(middle[3:last])[:r]
        elif i == nb - 3 or i == nb - 2:
            rand[i - 1, :] = rs.permutation(middle[:last])[:r]
        elif start > last:
            rand[i - 1, :] = rs.permutation(middle[:last])[:r]
        elif end + 1 == last:
            rand[i - 1, :] = rs.permutation(middle[:start])[:r]
        else:
            rand[i - 1, :] = rs.permutation(np.concatenate((middle[:start], middle[end + 1:last])))[:r]
    return rand


def _row_attention(rs, block_id: int, to_start: int, to_end: int, r: int) -> np.ndarray:
    """``_get_single_block_row_attention``: ``r`` random blocks of [to_start, to_end) for one query block, outside its
    window and the global blocks."""
    perm = rs.permutation(np.arange(to_start, to_end, dtype=np.int32))
    illegal = {block_id - 1, block_id, block_id + 1, 0, to_end - 1}
    if block_id == 1:
        illegal.add(to_end - 2)
    if block_id == to_end - 2:
        illegal.add(1)
    out = []
    for i in range(to_end - to_start):
        if int(perm[i]) not in illegal:
            out.append(perm[i])
        if len(out) == r:
            break
    return np.array(out, dtype=np.int32)


def _head_plan(rs, seq_length: int, block: int, heads: int, plan_len: list, plan_r: list, training: bool) -> list:
    """``_bigbird_block_rand_mask_with_head``: per head ``[seq_length / block - 2, sum(plan_r)]`` random blocks.  The
    draws interleave the heads, row by row, as transformers makes them."""
    nb = seq_length // block
    plan_blocks = np.array(plan_len) // block
    max_idx = plan_len.index(seq_length)
    rand = [np.zeros((nb, int(np.sum(plan_r[:max_idx + 1]))), dtype=np.int32) for _ in range(heads)]
    if training:
        for pi in range(max_idx + 1):
            lo = 0
            if pi > 0:
                if plan_r[pi] > 0:
                    lo, hi = int(np.sum(plan_r[:pi])), int(np.sum(plan_r[:pi + 1]))
                    for row in range(1, plan_blocks[pi - 1]):
                        for h in range(heads):
                            rand[h][row, lo:hi] = _row_attention(rs, row, plan_blocks[pi - 1], plan_blocks[pi],
                                                                 plan_r[pi])
                for pl in range(pi):
                    if plan_r[pl] == 0:
                        continue
                    for row in range(plan_blocks[pi - 1], plan_blocks[pi]):
                        lo, to_start = 0, 0
                        if pl > 0:
                            lo, to_start = int(np.sum(plan_r[:pl])), plan_blocks[pl - 1]
                        hi = int(np.sum(plan_r[:pl + 1]))
                        for h in range(heads):
                            rand[h][row, lo:hi] = _row_attention(rs, row, to_start, plan_blocks[pl], plan_r[pl])
            if plan_r[pi] == 0:
                continue
            hi = int(np.sum(plan_r[:pi + 1]))
            from_start, to_start = 1, 0
            if pi > 0:
                lo = int(np.sum(plan_r[:pi]))
                from_start = to_start = plan_blocks[pi - 1]
            for row in range(from_start, plan_blocks[pi]):
                for h in range(heads):
                    rand[h][row, lo:hi] = _row_attention(rs, row, to_start, plan_blocks[pi], plan_r[pi])
    return [x[1:nb - 1] for x in rand]


def bigbird_rand_blocks(seq_len: int, block_size: int, num_random_blocks: int, heads: int, seed: int, training: bool,
                        max_position_embeddings: int = 4096) -> np.ndarray:
    """The random blocks ``[heads, n - 2, num_random_blocks]`` transformers draws for query blocks 1 .. n - 2 of a
    sequence of ``seq_len`` tokens (n = ceil(seq_len / block_size): it pads to a block multiple first)."""
    n = -(-seq_len // block_size)
    padded = n * block_size
    rs = np.random.RandomState(seed)
    if padded in _OLD_PLAN_LENGTHS:
        rand = [_old_plan(rs, max_position_embeddings, block_size, num_random_blocks, training, 1024)[:n - 2]
                for _ in range(heads)]
    else:
        plan_len, plan_r = _rand_plan(padded, block_size, num_random_blocks)
        rand = _head_plan(rs, padded, block_size, heads, plan_len, plan_r, training)
    return np.stack(rand, axis=0)


def bigbird_plan(seq_len: int, block_size: int, num_random_blocks: int, heads: int, seed: int, training: bool,
                 max_position_embeddings: int = 4096) -> list:
    """Per head and per query block the list of key blocks BigBird attends to (module docstring), repeats kept: what
    :func:`..ops.attention.block_lists` takes, with ``block=block_size``."""
    n = -(-seq_len // block_size)
    if n < 5:
        raise ValueError(f"bigbird_plan: {seq_len} tokens are {n} blocks of {block_size}; the pattern needs at least 5 "
                         "(transformers runs full attention there)")
    rand = bigbird_rand_blocks(seq_len, block_size, num_random_blocks, heads, seed, training, max_position_embeddings)
    everything = list(range(n))
    plan = []
    for h in range(heads):
        rows = [everything]
        rows.append([0, 1, 2, n - 1] + [int(x) for x in rand[h, 0]])
        for i in range(2, n - 2):
            rows.append([0, i - 1, i, i + 1] + [int(x) for x in rand[h, i - 1]] + [n - 1])
        rows.append([0, n - 3, n - 2, n - 1] + [int(x) for x in rand[h, n - 3]])
        rows.append(everything)
        plan.append(rows)
    return plan


_plans: dict = {}


def cached_lists(seq_len: int, block_size: int, num_random_blocks: int, heads: int, layer: int, training: bool,
                 max_position_embeddings: int, device) -> BlockLists:
    """The :class:`BlockLists` of an encoder layer's pattern, kept per (layer, padded length, mode) — the plan depends
    on ``seq_len`` only through its number of blocks — with the kernels' tables uploaded when first built, so that a
    captured and replayed step builds and uploads nothing."""
    n = -(-seq_len // block_size)
    key = (layer, n, block_size, num_random_blocks, heads, bool(training), max_position_embeddings)
    bl = _plans.get(key)
    if bl is None:
        if len(_plans) > 256:
            _plans.clear()
        bl = block_lists(bigbird_plan(n * block_size, block_size, num_random_blocks, heads, layer, training,
                                      max_position_embeddings), block=block_size)
        _plans[key] = bl
    if block_size % 64 == 0 and getattr(device, "type", str(device)) != "cpu":
        bl.tables(device, seq_len, seq_len)
    return bl
