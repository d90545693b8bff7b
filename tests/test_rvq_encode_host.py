"""The float64 reference of the residual search (tests/rvq_encode_common.py) against the oracle's float32 search and against the codes the
third-party implementation produced (tests/golden/encodec.npz), on the cells where the reference itself is sure of its answer."""
import numpy as np

import rvq_encode_common as RC
from helpers import golden
from oracle import encodec_oracle as EO


def test_reference_agrees_with_oracle_and_golden_codes():
    g = golden("encodec")
    emb, tab = g["encoder.y"], RC.golden_tables(16)
    codes, clear = RC.search_ref(emb, tab)
    mask = RC.prefix_mask(clear)
    assert mask.mean() >= 0.95, mask.mean()
    assert np.array_equal(codes[mask], g["encoder.codes"][mask])
    assert np.array_equal(codes[mask], EO.rvq_encode(emb, tab)[mask])


def test_reference_on_scaled_tables_agrees_with_oracle():
    emb, tab = RC.frames(2, 75), RC.tables(16, 1024)
    codes, clear = RC.search_ref(emb, tab)
    mask = RC.prefix_mask(clear)
    assert mask.mean() >= 0.95, mask.mean()
    assert np.array_equal(codes[mask], EO.rvq_encode(emb, tab)[mask])


def test_validity_of_the_reference_itself_and_of_a_wrong_code():
    emb, tab = RC.frames(1, 17), RC.tables(2, 64)
    codes, _ = RC.search_ref(emb, tab)
    assert RC.validity(emb, tab, codes).max() <= 1.0
    wrong = codes.copy()
    wrong[1, 0, 3] = (wrong[1, 0, 3] + 1) % 64
    v = RC.validity(emb, tab, wrong)
    assert v[1, 0, 3] > 1.0 and v[0].max() <= 1.0


def test_prefix_mask_stops_at_the_first_unclear_layer():
    clear = np.array([[True, True], [False, True], [True, True]])
    assert RC.prefix_mask(clear).tolist() == [[True, True], [False, True], [False, True]]


def test_ties_go_to_the_lowest_index():
    tab = RC.tables(2, 128).copy()
    tab[1, 100] = tab[1, 5]
    emb = (tab[0, 7] + tab[1, 5])[None, :, None]
    codes, clear = RC.search_ref(emb, tab)
    assert codes[:, 0, 0].tolist() == [7, 5] and not clear[1, 0, 0]
