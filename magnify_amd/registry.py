"""Component / reader registries and the predefined pipelines.

Mirrors the reference's plugin API (src/magnify/registry.py): ``readers`` and ``components`` map a
name to a *factory*; ``factory(**kwargs)`` returns ``callable(Dataset) -> Dataset``.  Two
registration idioms exist and both are kept: ``@component("name")`` on ``f(xp, **kw)``
(registry.py:16-29) and ``@components.register("name")`` on a ``make(**kw)`` that returns a callable
object (stitch.py:48-50, find.py:404-442, 607-629).  The pipeline builders keep the reference's
keyword names and defaults verbatim (registry.py:32-59, 196-222, 454-470, 568-583, 615-621, 672-677).
"""
from __future__ import annotations

import functools
import inspect

from .utils import to_list


class Registry:
    """Minimal stand-in for a ``catalogue`` registry (register / get)."""

    def __init__(self, *namespace):
        self.namespace = namespace
        self._items = {}

    def register(self, name, func=None):
        def deco(f):
            self._items[name] = f
            return f

        return deco(func) if func is not None else deco

    def get(self, name):
        try:
            return self._items[name]
        except KeyError:
            avail = ", ".join(sorted(self._items))
            raise KeyError(f"Cant't find '{name}' in registry {' -> '.join(self.namespace)}. Available names: {avail}") from None

    def get_all(self):
        return dict(self._items)

    def __contains__(self, name):
        return name in self._items


readers = Registry("magnify", "readers")
components = Registry("magnify", "components")


class _Factory:
    """What ``component(name)`` puts into the registry for ``func(xp, **settings)``: calling it with the settings
    gives the pipeline step ``step(xp)``; it presents ``func``'s name, docstring and signature without the dataset
    parameter, which is what ``Pipeline.add_pipe(name, **settings)`` and introspection see (registry.py:16-29)."""

    def __init__(self, func):
        self._func = func
        functools.update_wrapper(self, func)
        dataset_param, *settings = inspect.signature(func).parameters.values()
        self.__signature__ = inspect.Signature(settings)

    def __call__(self, *args, **settings):
        func = self._func

        def step(xp, *more, **late):
            return func(*args, xp, *more, **{**settings, **late})

        step.__name__ = getattr(func, "__name__", "step")
        step.func, step.args, step.keywords = func, args, settings  # (what functools.partial would expose)
        return step


def component(name):
    """Decorator: register ``func(xp, **settings)`` under ``name``; ``func`` itself is returned unchanged, so a
    module can keep calling it directly."""

    def register(func):
        components.register(name)(_Factory(func))
        return func

    return register


from .pipeline import Pipeline  # noqa: E402  (Pipeline looks the registries up lazily)


def _add_segment(pipe, segment, channel, open_radius, max_grow, bg_guard, roi_length):
    """``segment=`` of the marker pipelines ("otsu" or a threshold; not in the reference): ``segment_rois`` directly
    after the finder, its settings checked now, not at the first assay.  None adds nothing."""
    if segment is None:
        return
    from .segment import check_segment

    check_segment(segment, open_radius, max_grow, bg_guard, roi_length=roi_length)
    pipe.add_pipe("segment_rois", method=segment, channel=channel, open_radius=open_radius, max_grow=max_grow,
                  bg_guard=bg_guard)


def _add_refine(pipe, refine, channel, rays, reach, polarity, roi_length):
    """``refine=`` of the marker pipelines ("edge"; not in the reference): ``refine_markers`` directly after the finder --
    before ``segment_rois`` and ``profile_rois`` -- its settings checked now, not at the first assay.  None adds nothing."""
    from .refine import check_method, check_refine

    if check_method(refine) is None:
        return
    check_refine(rays, reach, polarity, roi_length=roi_length)
    pipe.add_pipe("refine_markers", channel=channel, rays=rays, reach=reach, polarity=polarity)


def _add_profile(pipe, profile, rings, mask, roi_length):
    """``profile=`` of the marker pipelines (a ring width in pixels; not in the reference): ``profile_rois`` after the
    finder -- after ``segment_rois`` where that is present, so that the profile sees the final masks -- and before
    ``drop``, its settings checked now, not at the first assay.  None adds nothing."""
    if profile is None:
        return
    from .profile import check_profile

    check_profile(profile, rings, mask, roi_length)
    pipe.add_pipe("profile_rois", width=profile, rings=rings, mask=mask)


def _add_depth(pipe, depth, depth_window):
    """``depth=`` of the pipelines ("max", "mean", "sharpest" or "focus"; not in the reference, which refuses a Z
    axis): the reader keeps the files' Z axis as ``depth`` and ``project_depth`` folds it first, before
    ``standardize_format``; its settings are checked now, not at the first assay.  None changes nothing."""
    if depth is None:
        return
    from .depth import check_depth

    check_depth(depth, depth_window)
    pipe.reader = readers.get("read")(depth=True)
    pipe.add_pipe("project_depth", first=True, method=depth, window=depth_window)


def _add_despeckle(pipe, despeckle, radius, which, scope):
    """``despeckle=`` of the pipelines (a threshold in pixel units; not in the reference): ``remove_outliers`` directly
    after ``standardize_format`` -- on the raw tiles, before the flat-field maxima, the stitch and the finders -- its
    settings checked now, not at the first assay.  None adds nothing."""
    if despeckle is None:
        return
    from .despeckle import check_despeckle

    check_despeckle(despeckle, radius, which, scope)
    pipe.add_pipe("remove_outliers", after="standardize_format", threshold=despeckle, radius=radius, which=which,
                  scope=scope)


def _add_background(pipe, background, smooth, channel, after="stitch"):
    """``background=`` of the pipelines (the radius of the opening's window; not in the reference):
    ``subtract_background`` directly after ``after`` -- on the stitched (on the chip: stitched and rotated) image, so
    that no tile border lies inside a window -- its settings checked now, not at the first assay.  None adds nothing."""
    if background is None:
        return
    from .background import check_background

    check_background(background, smooth, channel)
    pipe.add_pipe("subtract_background", after=after, radius=background, smooth=smooth, channel=channel)


def _add_rotate(pipe, rotation, feature, max_angle, channel, min_confidence, time=0):
    """``rotate`` with ``rotation=``: a number of degrees as it was, the step's other settings at their defaults, or
    "auto" (not in the reference) with the settings of the estimate, checked now, not at the first assay."""
    if not isinstance(rotation, str):
        pipe.add_pipe("rotate", rotation=rotation)
        return
    from .skew import check_rotation

    check_rotation(rotation, feature, max_angle, min_confidence)
    pipe.add_pipe("rotate", rotation=rotation, rotation_feature=feature, rotation_max=max_angle, rotation_channel=channel,
                  rotation_min_confidence=min_confidence, rotation_time=time)


def microfluidic_chip(data, shape=(8, 8), pinlist=None, blank=None, overlap=102, rotation=0, row_dist=375 / 1.61,
                      col_dist=400 / 1.61, chip_type=None, min_button_diameter=8, max_button_diameter=30,
                      chamber_diameter=60, top_chamber=None, left_chamber=None, low_edge_quantile=0.1,
                      high_edge_quantile=0.9, num_iter=5000000, min_roundness=0.2, cluster_penalty=50, roi_length=None,
                      progress_bar=False, search_timestep=0, search_channel=None, roi_only=False, drop_tiles=True,
                      interactive=False, blend=None,
                      register=None, max_shift=8, register_channel=None,
                      segment=None, segment_channel=None, segment_open=1, segment_grow=4, segment_guard=2,
                      depth=None, depth_window=9,
                      despeckle=None, despeckle_radius=1, despeckle_which="bright", despeckle_scope="plane",
                      background=None, background_smooth=0, background_channel=None,
                      profile=None, profile_rings=None, profile_mask="own",
                      refine=None, refine_channel=None, refine_rays=64, refine_reach=3, refine_polarity="auto",
                      rotation_feature=None, rotation_max=10.0, rotation_min_confidence=2.0):
    """registry.py:32-110 (``blend``: ``stitch``'s overlap blending; ``register``, ``max_shift``, ``register_channel``:
    its tile registration; ``rotation="auto"`` with ``rotation_feature``, ``rotation_max``, ``rotation_min_confidence``:
    ``rotate``'s estimate of the tilt -- none of them is in the reference)."""
    kw = dict(locals())
    kw.pop("data")
    return microfluidic_chip_pipe(**kw)(data=data)


def microfluidic_chip_pipe(shape=(8, 8), pinlist=None, blank=None, overlap=102, rotation=0, row_dist=375 / 1.61,
                           col_dist=400 / 1.61, chip_type=None, min_button_diameter=8, max_button_diameter=30,
                           chamber_diameter=60, top_chamber=None, left_chamber=None, low_edge_quantile=0.1,
                           high_edge_quantile=0.9, num_iter=5000000, min_roundness=0.2, cluster_penalty=50,
                           roi_length=None, progress_bar=False, search_timestep=0, search_channel=None,
                           roi_only=False, drop_tiles=True, interactive=False, blend=None,
                           register=None, max_shift=8, register_channel=None,
                           segment=None, segment_channel=None, segment_open=1, segment_grow=4, segment_guard=2,
                           depth=None, depth_window=9,
                           despeckle=None, despeckle_radius=1, despeckle_which="bright", despeckle_scope="plane",
                           background=None, background_smooth=0, background_channel=None,
                           profile=None, profile_rings=None, profile_mask="own",
                           refine=None, refine_channel=None, refine_rays=64, refine_reach=3, refine_polarity="auto",
                           rotation_feature=None, rotation_max=10.0, rotation_min_confidence=2.0):
    """registry.py:196-271."""
    if chip_type is not None:
        if chip_type == "minichip":
            row_dist, col_dist = 375 / 1.61, 400 / 1.61
        elif chip_type == "pc":
            row_dist, col_dist = 406 / 3.22, 750 / 3.22
        elif chip_type == "ps":
            row_dist, col_dist = 375 / 3.22, 655 / 3.22
        else:
            raise ValueError(f"Invalid chip type: {chip_type}. Must be one of ['pc', 'ps', 'minichip']")
    pipe = Pipeline("read")
    pipe.add_pipe("standardize_format")
    _add_depth(pipe, depth, depth_window)
    _add_despeckle(pipe, despeckle, despeckle_radius, despeckle_which, despeckle_scope)
    pipe.add_pipe("identify_buttons", shape=shape, pinlist=pinlist, blank=blank)
    pipe.add_pipe("stitch", overlap=overlap, blend=blend, register=register, max_shift=max_shift,
                  register_channel=register_channel)
    _add_rotate(pipe, rotation, min_button_diameter if rotation_feature is None else rotation_feature, rotation_max,
                next(iter(to_list(search_channel)), None), rotation_min_confidence,
                min(to_list(search_timestep), default=0))
    _add_background(pipe, background, background_smooth, background_channel, after="rotate")
    pipe.add_pipe("find_buttons", row_dist=row_dist, col_dist=col_dist, min_button_diameter=min_button_diameter,
                  max_button_diameter=max_button_diameter, chamber_diameter=chamber_diameter, top_chamber=top_chamber,
                  left_chamber=left_chamber, low_edge_quantile=low_edge_quantile,
                  high_edge_quantile=high_edge_quantile, num_iter=num_iter, min_roundness=min_roundness,
                  cluster_penalty=cluster_penalty, roi_length=roi_length, progress_bar=progress_bar,
                  search_timestep=search_timestep, search_channel=search_channel, interactive=interactive)
    _add_refine(pipe, refine, next(iter(to_list(search_channel)), None) if refine_channel is None else refine_channel,
                refine_rays, refine_reach, refine_polarity, roi_length)
    _add_segment(pipe, segment, segment_channel, segment_open, segment_grow, segment_guard, roi_length)
    _add_profile(pipe, profile, profile_rings, profile_mask, roi_length)
    pipe.add_pipe("drop", roi_only=roi_only, drop_tiles=drop_tiles)
    pipe.add_pipe("restore_format")
    return pipe


def mrbles(data, spectra, codes, flatfield=1.0, darkfield=0.0, overlap=102, min_bead_diameter=10, max_bead_diameter=50,
           low_edge_quantile=0.1, high_edge_quantile=0.9, num_iter=5000000, min_roundness=0.3, roi_length=None,
           search_channel=None, reference="eu", roi_only=False, drop_tiles=True, interactive=False, blend=None,
           register=None, max_shift=8, register_channel=None,
           track=None, max_drift=8, track_min_score=0.5, track_channel=None, track_patch=None,
           stage_drift=None,
           segment=None, segment_channel=None, segment_open=1, segment_grow=4, segment_guard=2,
           depth=None, depth_window=9,
           despeckle=None, despeckle_radius=1, despeckle_which="bright", despeckle_scope="plane",
           background=None, background_smooth=0, background_channel=None,
           refine=None, refine_channel=None, refine_rays=64, refine_reach=3, refine_polarity="auto",
           profile=None, profile_rings=None, profile_mask="own", unmix=None):
    """registry.py:274-399 (``unmix``: ``identify_mrbles``' per-pixel unmixing; ``refine``: ``refine_markers``' sub-pixel
    circles; neither is in the reference)."""
    kw = dict(locals())
    kw.pop("data")
    return mrbles_pipe(**kw)(data=data)


def mrbles_pipe(spectra, codes, flatfield=1.0, darkfield=0.0, overlap=102, min_bead_diameter=10, max_bead_diameter=50,
                low_edge_quantile=0.1, high_edge_quantile=0.9, num_iter=5000000, min_roundness=0.3, roi_length=None,
                search_channel=None, reference="eu", roi_only=False, drop_tiles=True, interactive=False, blend=None,
                register=None, max_shift=8, register_channel=None,
                track=None, max_drift=8, track_min_score=0.5, track_channel=None, track_patch=None,
                stage_drift=None,
                segment=None, segment_channel=None, segment_open=1, segment_grow=4, segment_guard=2,
                depth=None, depth_window=9,
                despeckle=None, despeckle_radius=1, despeckle_which="bright", despeckle_scope="plane",
                background=None, background_smooth=0, background_channel=None,
                refine=None, refine_channel=None, refine_rays=64, refine_reach=3, refine_polarity="auto",
                profile=None, profile_rings=None, profile_mask="own", unmix=None):
    """registry.py:402-451."""
    from .unmix import check_unmix

    check_unmix(unmix)  # now, not at the first assay
    pipe = Pipeline("read")
    pipe.add_pipe("standardize_format")
    _add_depth(pipe, depth, depth_window)
    _add_despeckle(pipe, despeckle, despeckle_radius, despeckle_which, despeckle_scope)
    pipe.add_pipe("flatfield_correct", flatfield=flatfield, darkfield=darkfield)
    pipe.add_pipe("stitch", overlap=overlap, blend=blend, register=register, max_shift=max_shift,
                  register_channel=register_channel)
    _add_background(pipe, background, background_smooth, background_channel)
    pipe.add_pipe("find_beads", min_bead_diameter=min_bead_diameter, max_bead_diameter=max_bead_diameter,
                  low_edge_quantile=low_edge_quantile, high_edge_quantile=high_edge_quantile, num_iter=num_iter,
                  min_roundness=min_roundness, roi_length=roi_length, search_channel=search_channel,
                  interactive=interactive, track=track, max_drift=max_drift, track_min_score=track_min_score,
                  track_channel=track_channel, track_patch=track_patch, stage_drift=stage_drift)
    _add_refine(pipe, refine, next(iter(to_list(search_channel)), None) if refine_channel is None else refine_channel,
                refine_rays, refine_reach, refine_polarity, roi_length)
    _add_segment(pipe, segment, segment_channel, segment_open, segment_grow, segment_guard, roi_length)
    _add_profile(pipe, profile, profile_rings, profile_mask, roi_length)
    pipe.add_pipe("identify_mrbles", spectra=spectra, codes=codes, reference=reference, unmix=unmix)
    pipe.add_pipe("drop", roi_only=roi_only, drop_tiles=drop_tiles)
    pipe.add_pipe("restore_format")
    return pipe


def beads(data, flatfield=1.0, darkfield=0.0, overlap=102, min_bead_diameter=10, max_bead_diameter=50,
          low_edge_quantile=0.1, high_edge_quantile=0.9, num_iter=5000000, min_roundness=0.3, roi_length=None,
          search_channel=None, roi_only=False, drop_tiles=True, interactive=False, blend=None,
          register=None, max_shift=8, register_channel=None,
          track=None, max_drift=8, track_min_score=0.5, track_channel=None, track_patch=None,
          stage_drift=None,
          segment=None, segment_channel=None, segment_open=1, segment_grow=4, segment_guard=2,
          depth=None, depth_window=9,
          despeckle=None, despeckle_radius=1, despeckle_which="bright", despeckle_scope="plane",
          background=None, background_smooth=0, background_channel=None,
          refine=None, refine_channel=None, refine_rays=64, refine_reach=3, refine_polarity="auto",
          profile=None, profile_rings=None, profile_mask="own"):
    """registry.py:454-565."""
    kw = dict(locals())
    kw.pop("data")
    return beads_pipe(**kw)(data=data)


def beads_pipe(flatfield=1.0, darkfield=0.0, overlap=102, min_bead_diameter=5, max_bead_diameter=25,
               low_edge_quantile=0.1, high_edge_quantile=0.9, num_iter=5000000, min_roundness=0.3, roi_length=None,
               search_channel=None, roi_only=False, drop_tiles=True, interactive=False, blend=None,
               register=None, max_shift=8, register_channel=None,
               track=None, max_drift=8, track_min_score=0.5, track_channel=None, track_patch=None,
               stage_drift=None,
               segment=None, segment_channel=None, segment_open=1, segment_grow=4, segment_guard=2,
               depth=None, depth_window=9,
               despeckle=None, despeckle_radius=1, despeckle_which="bright", despeckle_scope="plane",
               background=None, background_smooth=0, background_channel=None,
               refine=None, refine_channel=None, refine_rays=64, refine_reach=3, refine_polarity="auto",
               profile=None, profile_rings=None, profile_mask="own"):
    """registry.py:568-612 (note the 5/25 defaults here versus 10/50 in ``beads``)."""
    pipe = Pipeline("read")
    pipe.add_pipe("standardize_format")
    _add_depth(pipe, depth, depth_window)
    _add_despeckle(pipe, despeckle, despeckle_radius, despeckle_which, despeckle_scope)
    pipe.add_pipe("flatfield_correct", flatfield=flatfield, darkfield=darkfield)
    pipe.add_pipe("stitch", overlap=overlap, blend=blend, register=register, max_shift=max_shift,
                  register_channel=register_channel)
    _add_background(pipe, background, background_smooth, background_channel)
    pipe.add_pipe("find_beads", min_bead_diameter=min_bead_diameter, max_bead_diameter=max_bead_diameter,
                  low_edge_quantile=low_edge_quantile, high_edge_quantile=high_edge_quantile, num_iter=num_iter,
                  min_roundness=min_roundness, roi_length=roi_length, search_channel=search_channel,
                  interactive=interactive, track=track, max_drift=max_drift, track_min_score=track_min_score,
                  track_channel=track_channel, track_patch=track_patch, stage_drift=stage_drift)
    _add_refine(pipe, refine, next(iter(to_list(search_channel)), None) if refine_channel is None else refine_channel,
                refine_rays, refine_reach, refine_polarity, roi_length)
    _add_segment(pipe, segment, segment_channel, segment_open, segment_grow, segment_guard, roi_length)
    _add_profile(pipe, profile, profile_rings, profile_mask, roi_length)
    pipe.add_pipe("drop", roi_only=roi_only, drop_tiles=drop_tiles)
    pipe.add_pipe("restore_format")
    return pipe


def blobs(data, flatfield=1.0, darkfield=0.0, overlap=102, threshold="otsu", search_channel=None, polarity="bright",
          smooth=False, connectivity=8, fill_holes=False, min_area=20, max_area=None, clear_border=False, roi_length=None,
          max_components=1 << 20, roi_only=False, drop_tiles=True, blend=None,
          register=None, max_shift=8, register_channel=None,
          depth=None, depth_window=9,
          despeckle=None, despeckle_radius=1, despeckle_which="bright", despeckle_scope="plane",
          background=None, background_smooth=0, background_channel=None,
          profile=None, profile_rings=None, profile_mask="own"):
    """Markers of any shape (not in the reference): ``beads`` with ``find_blobs`` (blobs.py) in the finder's place."""
    kw = dict(locals())
    kw.pop("data")
    return blobs_pipe(**kw)(data=data)


def blobs_pipe(flatfield=1.0, darkfield=0.0, overlap=102, threshold="otsu", search_channel=None, polarity="bright",
               smooth=False, connectivity=8, fill_holes=False, min_area=20, max_area=None, clear_border=False,
               roi_length=None, max_components=1 << 20, roi_only=False, drop_tiles=True, blend=None,
               register=None, max_shift=8, register_channel=None,
               depth=None, depth_window=9,
               despeckle=None, despeckle_radius=1, despeckle_which="bright", despeckle_scope="plane",
               background=None, background_smooth=0, background_channel=None,
               profile=None, profile_rings=None, profile_mask="own"):
    """read -> standardize_format -> depth -> despeckle -> flatfield_correct -> stitch -> background -> find_blobs ->
    profile -> drop -> restore_format; the finder's settings are checked now, not at the first assay."""
    from .blobs import check_blobs

    check_blobs(threshold, search_channel, polarity, smooth, connectivity, fill_holes, min_area, max_area, clear_border,
                roi_length, max_components)
    pipe = Pipeline("read")
    pipe.add_pipe("standardize_format")
    _add_depth(pipe, depth, depth_window)
    _add_despeckle(pipe, despeckle, despeckle_radius, despeckle_which, despeckle_scope)
    pipe.add_pipe("flatfield_correct", flatfield=flatfield, darkfield=darkfield)
    pipe.add_pipe("stitch", overlap=overlap, blend=blend, register=register, max_shift=max_shift,
                  register_channel=register_channel)
    _add_background(pipe, background, background_smooth, background_channel)
    pipe.add_pipe("find_blobs", threshold=threshold, search_channel=search_channel, polarity=polarity, smooth=smooth,
                  connectivity=connectivity, fill_holes=fill_holes, min_area=min_area, max_area=max_area,
                  clear_border=clear_border, roi_length=roi_length, max_components=max_components)
    _add_profile(pipe, profile, profile_rings, profile_mask, roi_length)
    pipe.add_pipe("drop", roi_only=roi_only, drop_tiles=drop_tiles)
    pipe.add_pipe("restore_format")
    return pipe


def image(data, overlap=102, rotation=0, roi_only=False, drop_tiles=True, blend=None,
          register=None, max_shift=8, register_channel=None, depth=None, depth_window=9,
          despeckle=None, despeckle_radius=1, despeckle_which="bright", despeckle_scope="plane",
          background=None, background_smooth=0, background_channel=None,
          rotation_feature=16, rotation_max=10.0, rotation_channel=None, rotation_min_confidence=2.0):
    """registry.py:615-669."""
    return image_pipe(overlap=overlap, rotation=rotation, roi_only=roi_only, drop_tiles=drop_tiles, blend=blend,
                      rotation_feature=rotation_feature, rotation_max=rotation_max, rotation_channel=rotation_channel,
                      rotation_min_confidence=rotation_min_confidence,
                      register=register, max_shift=max_shift, register_channel=register_channel, depth=depth,
                      depth_window=depth_window, despeckle=despeckle, despeckle_radius=despeckle_radius,
                      despeckle_which=despeckle_which, despeckle_scope=despeckle_scope, background=background,
                      background_smooth=background_smooth, background_channel=background_channel)(data=data)


def image_pipe(overlap=102, rotation=0, roi_only=False, drop_tiles=True, blend=None,
               register=None, max_shift=8, register_channel=None, depth=None, depth_window=9,
               despeckle=None, despeckle_radius=1, despeckle_which="bright", despeckle_scope="plane",
               background=None, background_smooth=0, background_channel=None,
               rotation_feature=16, rotation_max=10.0, rotation_channel=None, rotation_min_confidence=2.0):
    """registry.py:672-693."""
    pipe = Pipeline("read")
    pipe.add_pipe("standardize_format")
    _add_depth(pipe, depth, depth_window)
    _add_despeckle(pipe, despeckle, despeckle_radius, despeckle_which, despeckle_scope)
    pipe.add_pipe("stitch", overlap=overlap, blend=blend, register=register, max_shift=max_shift,
                  register_channel=register_channel)
    _add_background(pipe, background, background_smooth, background_channel)
    _add_rotate(pipe, rotation, rotation_feature, rotation_max, rotation_channel, rotation_min_confidence)
    pipe.add_pipe("drop", roi_only=roi_only, drop_tiles=drop_tiles)
    pipe.add_pipe("restore_format")
    return pipe
