"""The door texts of the three row sources (misti_bootstrap_rows_dev, misti_jackknife_rows_dev, misti_parametric_rows_dev) where they
meet the context, whole text for whole text: valid arguments without a context end at exactly "ctx is NULL", and a chunk table with a
bad entry is refused for that entry although the context is missing too - the arguments are judged before the context is looked at."""
import pytest

import test_bootstrap_rows_cpu as boot
import test_jackknife_rows_cpu as jack
import test_parametric_rows_cpu as parametric

E_ARG = -1


@pytest.mark.parametrize("door", [lambda: boot.rows_dev(boot.GOOD), lambda: jack.rows_dev(jack.GOOD), parametric.rows_dev],
                         ids=["bootstrap", "jackknife", "parametric"])
def test_valid_arguments_without_a_context_end_at_the_context(door):
    rc, why = door()
    assert rc == E_ARG and why == "ctx is NULL", (rc, why)


@pytest.mark.parametrize("source", [boot, jack], ids=["bootstrap", "jackknife"])
def test_the_chunk_refusal_comes_before_the_context(source):
    rc, why = source.rows_dev(source.bad(1, 0, 0.0))
    assert rc == E_ARG and why == "chunks[1][0] = 0: a chunk's length must be > 0", (rc, why)
