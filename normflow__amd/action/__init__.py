from .scalar_action import ScalarPhi4Action, ScalarPhi4Ladder
