from peekvit_amd.models.eeresidualvit import *  # noqa: F401,F403
from peekvit_amd.models import eeresidualvit as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
