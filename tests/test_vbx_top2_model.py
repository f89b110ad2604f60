"""CPU: the rule of VBx's second speaker (tests/vbx_top2_model.py) at the places a kernel can get it wrong."""
import numpy as np

import vbx_top2_model as V


def test_ties_go_to_the_smallest_speaker():
    g = np.asarray([[0.25, 0.25, 0.25, 0.25],
                    [0.1, 0.4, 0.4, 0.1],
                    [0.3, 0.1, 0.3, 0.3],
                    [0.0, 0.0, 0.5, 0.5]])
    labels, k, labels2, post2 = V.top2(g)
    # first: 0, 1, 0, 2 -> alive {0, 1, 2} (3 is nobody's first), numbered 0, 1, 2 by first member (rows 0, 1, 3)
    assert labels.tolist() == [0, 1, 0, 2] and k == 3
    # second: row 0 ties 1 = 2 -> 1; row 1 ties 2 (0.4) -> 2; row 2 ties 2 = 3 but 3 is dead -> 2; row 3: 0 = 1 = 0.0 -> 0
    assert labels2.tolist() == [1, 2, 2, 0] and post2.tolist() == [0.25, 0.4, 0.3, 0.0]


def test_a_dead_speaker_with_the_highest_runner_up_is_skipped():
    g = np.asarray([[0.50, 0.45, 0.05],
                    [0.48, 0.47, 0.05],
                    [0.05, 0.45, 0.50],
                    [0.02, 0.49, 0.49 + 2 ** -40]])
    labels, k, labels2, post2 = V.top2(g)
    assert labels.tolist() == [0, 0, 1, 1] and k == 2                     # speaker 1 is the runner-up of every row, and dead
    assert labels2.tolist() == [1, 1, 0, 0]
    assert post2.tolist() == [0.05, 0.05, 0.05, 0.02]                     # entries of gamma, not recomputed


def test_renumbering_follows_the_first_member():
    g = np.asarray([[0.1, 0.2, 0.7], [0.6, 0.3, 0.1], [0.2, 0.1, 0.7]])
    labels, k, labels2, post2 = V.top2(g)
    assert labels.tolist() == [0, 1, 0] and k == 2                        # speaker 2 first (row 0), then speaker 0; 1 is dead
    assert labels2.tolist() == [1, 0, 1] and post2.tolist() == [0.1, 0.1, 0.2]


def test_one_speaker():
    for g in (np.ones((1, 1)), np.ones((5, 1)), np.asarray([[0.9, 0.1], [0.8, 0.2]])):
        labels, k, labels2, post2 = V.top2(g)
        assert k == 1 and (labels == 0).all() and (labels2 == -1).all() and (post2 == 0.0).all()
        assert labels2.dtype == np.int32 and post2.dtype == np.float64
