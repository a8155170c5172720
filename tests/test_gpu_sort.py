"""The radix sort, the splitter search and the rank scatter of csrc/bk_sort.hip on the MI355X, bit for bit: every class of
double through the key image, passes in which one digit holds every key, tile counts around the eight XCDs and the chunk
seam with full-width payloads, skewed digits, the scan's carry across one, two and three rounds (16.8 M keys), the work
buffer's and the outputs' edges with the refusals, bk_count_below on long runs and NaN, bk_scatter_ranks, and the pooled
ranks against NumPy on NaNs of both signs.  The bodies and their references: tests/sort_parity.py."""
import pytest

import bayes_kit_amd as bk
from tests import sort_parity as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


@pytest.mark.parametrize("n", sp.KEY_IMAGE_SIZES)
def test_key_image_on_every_class_of_double(ops, n):
    sp.check_key_image(ops, n)


@pytest.mark.parametrize("n", sp.SINGLE_BYTE_SIZES)
def test_passes_in_which_one_digit_holds_every_key(ops, n):
    sp.check_single_byte_passes(ops, n)


@pytest.mark.parametrize("n", sp.SEAM_SIZES)
def test_tile_counts_chunk_seam_and_full_width_payloads(ops, n):
    sp.check_tile_and_chunk_seams(ops, n)


def test_skewed_digits(ops):
    sp.check_skewed_digits(ops)


@pytest.mark.parametrize("mode", sp.SCAN_MODES)
@pytest.mark.parametrize("tiles", sp.SCAN_TILES)
def test_scan_carry_across_rounds(ops, tiles, mode):
    sp.check_scan_rounds(ops, tiles, mode)


def test_work_buffer_output_views_and_refusals(ops):
    sp.check_work_buffer_and_views(ops)


def test_count_below_on_runs_neighbours_and_nan(ops):
    sp.check_count_below(ops)


def test_scatter_ranks(ops):
    sp.check_scatter_ranks(ops)


def test_pooled_ranks_against_numpy(ops):
    sp.check_pooled_ranks_against_numpy(ops)
