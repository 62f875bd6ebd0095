"""Drop-in for frozenlake/FrozenLakeNet.py."""
from azhip.frozenlake import FrozenLakeNet  # noqa: F401
