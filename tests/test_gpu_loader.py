"""GameplayLoader.load_pool on the MI355X where its store encodes in several launches (mortal_amd/dataset.py _load,
load_batch_rows).  The case lives in tests/loader_cases.py, shared with the host-emulation leg (tests/test_emu_loader.py)."""
import pytest

import loader_cases as LC
import pool_gameplay_cases as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def played():
    """Two finished games and their logs as the host reads them, shared and left unchanged."""
    from mortal_amd.pool import TablePool

    pool = G.play(TablePool, 2)
    yield pool, pool.read_logs()
    pool.close()


@pytest.mark.parametrize("version,seats", [(3, (15, 15)), (4, (4, 2))])  # (obs v4: one seat a table keeps the reference's side quick)
def test_more_samples_than_one_encode_launch_takes(oracle, played, version, seats):
    assert LC.check_chunked(oracle, *played, version, seats) > 4 * LC.load_batch_rows(2)  # (at least four full launches)
