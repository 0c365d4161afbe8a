"""CounTR on the MI355X.  The raw-frame entry points, the device augmentation and the evaluation report are re-exported here; they load on first use so that `import countr_amd` (the
build, the CPU tools) stays free of torch."""


def __getattr__(name):
    if name in ("count_frames", "locate_frames", "count_regions", "count_classes", "ClassCounts", "FramePrep", "annotate_frames", "count_clip",
                "count_flow", "annotate_clip"):
        from . import frames
        return getattr(frames, name)
    if name in ("flow_host", "FlowCounter", "FlowCounts", "blob_scene"):
        from . import flow
        return getattr(flow, name)
    if name in ("camera_host", "texture_host", "estimate_host", "compensate_host", "CameraEstimator", "CameraPath", "pan_scene"):
        from . import cam
        return getattr(cam, name)
    if name in ("Overlay", "overlay_host"):
        from . import overlay
        return getattr(overlay, name)
    if name in ("draw_host", "Marks", "Painter", "Trails", "clip_marks", "track_color", "PALETTE"):
        from . import draw
        return getattr(draw, name)
    if name in ("tracks_host", "Tracker", "ClipCounts"):
        from . import tracks
        return getattr(tracks, name)
    if name in ("PeakFinder", "peaks_host", "Peaks"):
        from . import peaks
        return getattr(peaks, name)
    if name in ("RegionSummer", "regions_host"):
        from . import regions
        return getattr(regions, name)
    if name in ("ClassFolder", "classes_host"):
        from . import classes
        return getattr(classes, name)
    if name in ("TileStitcher", "tiles_host", "tile_starts"):
        from . import tiles
        return getattr(tiles, name)
    if name in ("YuvFrame", "YuvConverter", "yuv_host"):
        from . import yuv
        return getattr(yuv, name)
    if name in ("match_host", "PointMatcher", "localization_metrics", "LocalizationTotals"):
        from . import match
        return getattr(match, name)
    if name in ("count_carpk", "CarpkPrep"):
        from . import carpk
        return getattr(carpk, name)
    if name == "DeviceAug":
        from . import device_aug
        return device_aug.DeviceAug
    if name == "PretrainAug":
        from . import pretrain_aug
        return pretrain_aug.PretrainAug
    if name in ("ReportWriter", "ReportItem", "compose_host", "exemplar_strip_host"):
        from . import report
        return getattr(report, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
