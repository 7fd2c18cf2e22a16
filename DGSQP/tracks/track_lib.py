"""Reference path DGSQP/tracks/track_lib.py (``StraightTrack`` :14, ``CurveTrack`` :27, ``ChicaneTrack`` :54, ``get_track`` :96,
``load_mpclab_raceline`` :124, ``load_tum_raceline`` :145) -> dgsqp_amd.tracks.  The scripts use ``from DGSQP.tracks.track_lib import *``."""
from dgsqp_amd.tracks import (RadiusArclengthTrack, StraightTrack, CurveTrack, ChicaneTrack, CubicSplineTrack, get_track,  # noqa: F401
                              load_mpclab_raceline, load_tum_raceline)
__all__ = ['RadiusArclengthTrack', 'StraightTrack', 'CurveTrack', 'ChicaneTrack', 'CubicSplineTrack', 'get_track', 'load_mpclab_raceline',
           'load_tum_raceline']
