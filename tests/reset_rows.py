"""The row rule of rp_set_reset_table: which table row each env that ends in one rp_step_autoreset call starts its new episode from.

The ended env e takes row (cursor + rank(e)) mod rows, where rank(e) counts the ended envs with a smaller index in the same call and cursor is the
handle's cursor when the call began; the cursor then moves on by the number of ends, mod rows.  Envs that did not end get -1.
"""
import numpy as np


def reset_rows(done, cursor, rows):
    """done: [N] bools / ints of one call; returns (int32 [N] rows, -1 where done is 0; the cursor after the call)"""
    done = np.asarray(done).reshape(-1) != 0
    rank = np.cumsum(done) - done
    out = np.where(done, (cursor + rank) % rows, -1).astype(np.int32)
    return out, int((cursor + int(done.sum())) % rows)
