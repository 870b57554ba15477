# reference models/rankpct.py: RankPointCloudTransformer - and PointCloudTransformer, which the reference's configs/model/pct.yaml names here
from peekvit_amd.models.pct import *  # noqa: F401,F403
from peekvit_amd.models import pct as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
PCTEncoder = _impl.RankPCTEncoder          # (the reference's rankpct.py calls its ranking encoder PCTEncoder)
