"""The table of tests/test_xf_plan_host.py as lines for tools/xf_plan_check.cpp: `switches (3)  case (8)  expected row (11)`."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import test_xf_plan_host as T

for _, geom, hw, fp8, bx, shared, env, forms, plan in T.TABLE:
  print(*env, *geom, hw, fp8, bx, shared, *forms, *plan)
