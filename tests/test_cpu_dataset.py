"""Channel name or index -> index, the one lookup of the finders, the filters and segment_rois."""
import numpy as np
import pytest


def dataset(names):
    import magnify_amd as mg

    coords = {"channel": np.array(names)} if names else None
    return mg.Dataset({"roi": mg.DataArray(np.zeros((1, 2, 1, 3, 3), dtype=np.uint16),
                                           ("mark", "channel", "time", "roi_y", "roi_x"))}, coords=coords)


@pytest.mark.parametrize("names, channel, want", [(["dapi", "cy5"], "cy5", 1), (["dapi", "cy5"], 1, 1),
                                                  (["dapi", "cy5"], np.int64(0), 0), (None, 1, 1)])
def test_channel_index_accepts(names, channel, want):
    from magnify_amd import _dataset, segment

    got = _dataset.channel_index(dataset(names), channel)
    assert got == want and type(got) is int
    assert segment.channel_index(dataset(names), channel) == want
    assert _dataset.channel_indexes(dataset(names), channel) == [want]
    assert _dataset.channel_indexes(dataset(names), [channel, channel]) == [want, want]


def test_none_gives_the_default_or_every_channel():
    from magnify_amd import _dataset, segment

    ds = dataset(["dapi", "cy5"])
    assert _dataset.channel_index(ds, None, default=0) == 0 and _dataset.channel_index(ds, None) is None
    assert segment.channel_index(ds, None) == 0
    assert _dataset.channel_indexes(ds, None) == [0, 1]


@pytest.mark.parametrize("names, channel", [(["dapi", "cy5"], "gfp"), (["dapi", "cy5"], 2), (["dapi", "cy5"], -1),
                                            (["dapi", "cy5"], True), (None, "cy5"), (None, 2)])
@pytest.mark.parametrize("caught", [KeyError, ValueError])
def test_a_miss_is_a_key_error_and_a_value_error(names, channel, caught):
    from magnify_amd import _dataset, segment

    for lookup in (_dataset.channel_index, segment.channel_index, lambda ds, c: _dataset.channel_indexes(ds, [c])):
        with pytest.raises(caught):
            lookup(dataset(names), channel)
