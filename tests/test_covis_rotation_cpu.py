"""The rotation of tests/test_gpu_covis_rotation.py on the models alone (tests/rotation_case.py): the sequence runs, and it is not vacuous — at every row length
a keyframe is culled and one is kept, points go bad through the culls, a refresh chooses a descriptor and refuses an entry, and the second refresh differs
from the first because of the culls between them."""
import pytest

import rotation_case as RC


@pytest.mark.parametrize("L", RC.LENGTHS)
def test_rotation_is_not_vacuous_on_the_models(L):
    c = RC.make_case(L)
    b = RC.model_only()
    RC.load(b, c)
    assert sorted(b.m.rows) == [k for k in RC.KIDS if k != RC.HOLE] and b.m.holes == 1
    assert all(len(r) == L for r in b.m.rows.values())
    assert max(p for r in c.rows.values() for p in r) < RC.MAX_PTS
    if L >= 5:                                                      # NULLs, repeats and bad points inside the rows
        flat = [p for r in b.m.rows.values() for p in r]
        assert -1 in flat and RC.BAD0 in flat and any(len(set(r)) < len(r) for r in b.m.rows.values())
    log = RC.rotate(b, c)
    RC.assert_not_vacuous(c, log)
    end = b.m
    f = RC.fresh_copy(b, RC._ModelDev())
    f.d.b = f
    assert f.m.rows == end.rows and f.m.pt_bad == end.pt_bad and f.m.kf_bad == end.kf_bad
