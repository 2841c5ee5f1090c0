"""Float restatement of a window session (include/session/fsnp_window_stream.h), independent of the library: one slot simulated push by
push on top of the windowed call's own restatement (tests/_windowed_util.py: window_plan, merge).  Shared by
tests/test_host_window_stream.py and tests/test_gpu_window_stream.py."""
import numpy as np

from tests._windowed_util import merge, window_plan


class SlotSim:
    """One slot of a session at window W, overlap V.  enhance(samples) -> the enhanced window (default: the window itself).  Every
    contract property the simulation can see is asserted as it goes; `ran` lists (start, length) of the windows in the order they ran,
    `per_push` the (first, num) of the windows each push completed."""

    def __init__(self, W, V, enhance=None, dtype=np.float64):
        self.W, self.V, self.S, self.dtype = W, V, W - V, dtype
        self.enhance = enhance or (lambda x: np.asarray(x, dtype=dtype))
        self.x = np.zeros(0, dtype=dtype)          # every sample pushed
        self.rows, self.ran, self.per_push = [], [], []
        self.final = np.zeros(0, dtype=dtype)      # merged samples that no later window changes: [0, len(rows) S)

    @property
    def pushed(self):
        return len(self.x)

    def _run(self, start, n):
        self.rows.append(np.asarray(self.enhance(self.x[start:start + n]), dtype=self.dtype))
        self.ran.append((start, n))

    def push(self, block):
        """-> the len(block) output samples: merged sample P + j - W, 0 while that is negative"""
        W, V, S, P = self.W, self.V, self.S, self.pushed
        self.x = np.concatenate([self.x, np.asarray(block, dtype=self.dtype)])
        first = len(self.rows)
        while len(self.rows) * S + W <= self.pushed:                     # window k is complete at k S + W samples
            k = len(self.rows)
            self._run(k * S, W)
            if k == 0:
                seg = self.rows[0][:S]
            else:                                                        # [k S, (k + 1) S) of the clip = [S, 2 S) of the two windows' own merge
                seg = merge([self.rows[k - 1], self.rows[k]], S + W, W, V, self.dtype)[S:2 * S]
            self.final = np.concatenate([self.final, seg])
        self.per_push.append((first, len(self.rows) - first))
        out = np.zeros(len(block), dtype=self.dtype)
        lo, hi = max(0, P - W), self.pushed - W                          # the merged samples due now: [lo, hi)
        if hi > lo:
            assert hi <= len(self.final), f"outputs up to {hi} are due at {self.pushed} samples, but only {len(self.final)} merged samples exist"
            out[len(block) - (hi - lo):] = self.final[lo:hi]
        pending = len(self.final) - max(0, self.pushed - W)
        assert 0 <= pending <= S, f"{pending} merged samples wait, more than the stride {S}"
        return out

    def finish(self):
        """-> W samples: merged samples L - W .. L - 1 of the whole clip, 0 where the index is negative"""
        W, V, L = self.W, self.V, self.pushed
        plan = window_plan(L, W, V)
        assert self.ran == plan[:len(self.ran)] and all(n == W for _, n in self.ran), "the pushes ran exactly the plan's full windows"
        left = plan[len(self.ran):]
        assert len(left) <= 1, f"finish has {len(left)} windows left to run"
        for start, n in left:
            assert n > V or len(plan) == 1, f"the last window has {n} <= overlap {V} samples"
            self._run(start, n)
        full = merge(self.rows, L, W, V, self.dtype)
        assert np.array_equal(full[:len(self.final)], self.final), "a merged sample changed after it was final"
        out = np.zeros(W, dtype=self.dtype)
        n = min(W, L)
        out[W - n:] = full[L - n:]
        return out


def random_blocks(rng, total, largest, idle=0.15):
    """block sizes that sum to `total`: 1 ... largest each, with idle pushes (0) mixed in"""
    blocks, left = [], total
    while left > 0:
        if rng.random() < idle:
            blocks.append(0)
            continue
        c = int(min(left, rng.integers(1, largest + 1)))
        blocks.append(c)
        left -= c
    return blocks


def feed(session, clips, blocks_per_slot, n_cols, pad_value, dtype, channels=1, **push_kw):
    """Feed clips[b] (1-D CPU tensors) into slot b of a GPU session in blocks_per_slot[b] (one list of counts per slot, padded with
    idle pushes to one length; n_cols: None, or the width of every push), `pad_value` written past every count -> per slot, the
    concatenated live output columns of all pushes.  channels > 1: every block is channel 0 of a [slots, n, channels] interleaved
    buffer, read where it lies.  Also checks that columns past a slot's count are exactly 0."""
    import torch
    slots = len(clips)
    rounds = max(len(b) for b in blocks_per_slot)
    at = [0] * slots
    outs = [[] for _ in range(slots)]
    for r in range(rounds):
        counts = [blocks[r] if r < len(blocks) else 0 for blocks in blocks_per_slot]
        n = max(max(counts), 1) if n_cols is None else n_cols
        block = torch.full((slots, n), pad_value, dtype=dtype)
        for b, c in enumerate(counts):
            block[b, :c] = clips[b][at[b]:at[b] + c]
            at[b] += c
        if channels > 1:
            buf = torch.full((slots, n, channels), pad_value, dtype=dtype)
            buf[:, :, 0] = block
            block = buf.cuda()[:, :, 0]
            assert block.stride(1) == channels or n == 1
        got = session.push(block.cuda(), counts, **push_kw).cpu()
        for b, c in enumerate(counts):
            assert torch.count_nonzero(got[b, c:]) == 0, f"push {r}, slot {b}: columns past its count {c} are not 0"
            outs[b].append(got[b, :c])
    assert at == [len(c) for c in clips]
    return [torch.cat(o) for o in outs]
