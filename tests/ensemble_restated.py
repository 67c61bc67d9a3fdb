"""The per-pixel vote over K id maps, restated in numpy: the yardstick of premvos_idmap_vote_u8 (the reference has no vote: the
combination of MergeTrack/oldmerge.py:129-131,220-224's to_ensemble/<n>/ trees is not in its checkout).  A plain loop over the sets:
set k's count at a pixel is the number of sets that painted set k's label there; the largest count wins, the smallest k on a tie."""
import numpy as np


def vote(maps):
    """maps uint8 [K, ...] -> (voted uint8 [...], votes uint8 [...], hist int64 [K+1]: hist[v] = pixels whose winner has v votes)"""
    maps = np.asarray(maps, np.uint8)
    K = maps.shape[0]
    voted = np.zeros(maps.shape[1:], np.uint8)
    votes = np.zeros(maps.shape[1:], np.uint8)
    for k in range(K):
        count = np.zeros(maps.shape[1:], np.uint8)
        for j in range(K):
            count += maps[j] == maps[k]
        better = count > votes                      # strictly: an earlier set keeps a tie (and set 0 beats the initial 0)
        voted[better] = maps[k][better]
        votes[better] = count[better]
    return voted, votes, np.bincount(votes.reshape(-1), minlength=K + 1).astype(np.int64)
