"""The pure helpers the kernels inline (ihmr_amd/csrc/ihmr_pure.h) on NaN, +-inf, +-3e38, 1e30, -0.0 and an ordinary value, in a
stand-alone program (tests/nonfinite_driver.cpp) built with -fsanitize=address,undefined AND float-cast-overflow (GCC's `undefined`
group does not include the float-to-integer check).  The program feeds every helper the full cross product of those values in each
argument that carries caller data and counts the calls that break a rule; a sanitizer report aborts it.

What the audit of DESIGN.md ("Non-finite input") rests on, pinned here:
  * `in_grid` is false for any non-finite query or box, and the cell of an in-grid query lies in [-1, 31]^3 -- the only place where the
    samplers and the prep kernel turn a grid coordinate into an index;
  * `tri_col_range` (an unclamped float-to-int conversion) is reached only behind the yz-degeneracy test of a hand normalised by its OWN
    box, and there every coordinate has magnitude <= 1: its ranges are empty or inside [0, 31].  The degeneracy test alone would not do
    (a determinant of +-inf passes it): the count of such triangles is printed;
  * `sdf_ray_column_hits` sets no bit outside `need`, whatever the corners hold;
  * `align_root(NaN)` = -1 (no alignment: no lane index is formed from it).

Cost: the program makes 8^9 ray calls, 4 * 9^7 query calls and 2 * 8^7 box normalisations under the sanitizers: 3 s to build, 10 s to
run on one core (measured), once per module."""
import shutil

import pytest

import hostbuild

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

VALS = ("nan", "+inf", "-inf", "+3e38", "-3e38", "1e30", "-0.0", "0.37")


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    exe = hostbuild.build("nonfinite_driver.cpp", tmp_path_factory.mktemp("nonfinite"), hostbuild.X86_V3 + ["-fsanitize=float-cast-overflow"])
    r = hostbuild.run(exe)                               # exit status 0: no sanitizer report (-fno-sanitize-recover=all)
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    out = dict(line.split() for line in r.stdout.splitlines())
    print("[nonfinite host]", out)
    return {k: int(v) for k, v in out.items()}


def test_query_cell_is_in_grid_only_for_finite_arguments(counts):
    assert counts["query_calls"] == 4 * 9 ** 7                       # (query 3, centre 3, scale) from nine values x swap_xz x align_corners
    assert counts["query_in_grid"] > 1000, "no combination lands in the grid: the cell checks below would be vacuous"
    assert counts["query_in_grid_with_nonfinite_argument"] == 0
    assert counts["query_cell_outside_minus1_31"] == 0 and counts["query_bad_cell_word"] == 0
    assert counts["trilinear_calls"] == 8 * counts["query_in_grid"] and counts["grad_to_vertex_calls"] == 4 * 8 ** 4
    assert counts["corner_mask_calls"] == 64 * 4 and counts["corner_mask_bad"] == 0


def test_division_helper_keeps_the_plain_quotient_wherever_it_is_finite(counts):
    assert counts["div_calls"] == 64 and counts["div_differs_with_a_finite_quotient"] == 0
    # the fast form turns an overflowing quotient into NaN where the plain division gives +-inf (never a grid coordinate either way):
    # exactly the four pairs +-inf / 0.37 and +-3e38 / 0.37 (0.37 is the one divisor of the set inside the fast range)
    assert counts["div_differs_from_plain_division"] == 4


def test_column_range_is_reached_only_with_normalised_coordinates(counts):
    assert counts["prep_calls"] == 2 * 8 ** 7
    assert counts["prep_passed_det_test"] > 10000 and counts["prep_passed_det_test_with_nonfinite_vertex"] > 1000, \
        "hands with a non-finite vertex must reach the range computation, or the precondition is not exercised"
    assert counts["prep_normalised_above_one"] == 0, "a hand normalised by its own box handed tri_col_range a coordinate above 1"
    assert counts["prep_nonempty_ranges"] > 1000 and counts["prep_bad_range"] == 0
    assert counts["range_domain_calls"] == 9 ** 6 and counts["range_domain_bad"] == 0
    # why the precondition is the box and not the degeneracy test: the test alone lets non-finite triangles through
    assert counts["det_calls"] == 8 ** 6 and counts["det_test_alone_passes_nonfinite"] > 0


def test_ray_mask_stays_inside_need(counts):
    assert counts["ray_calls"] == 8 ** 9
    assert counts["ray_uv_passes"] > 1000 and counts["ray_with_hits"] > 100
    assert counts["ray_bits_outside_need"] == 0


def test_align_root_and_the_steps(counts):
    root = {v: counts[f"align_root_{i}"] for i, v in enumerate(VALS)}
    assert root["nan"] == -1 and root["0.37"] == -1
    assert root["+inf"] == root["+3e38"] == root["1e30"] == 0 and root["-inf"] == root["-3e38"] == root["-0.0"] == 21
    assert set(root.values()) <= {-1, 0, 21}
    assert counts["adam_calls"] == 8 ** 4 and counts["sgd_calls"] == 8 ** 3 and counts["rodrigues_bwd_calls"] == 8 ** 4
