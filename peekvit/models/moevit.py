from peekvit_amd.models.moevit import *  # noqa: F401,F403
from peekvit_amd.models import moevit as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
