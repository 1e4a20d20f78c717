#!/bin/bash
# tools/build_variant.sh <name> [extra hipcc flags...]  ->  forces_resilient_planner_amd/lib_<name>.so  (profile builds: -DFRP_PROFILE ...)
# The product sources with their per-source flags plus the extra flags.
set -e
cd "$(dirname "$0")/.."
python -m forces_resilient_planner_amd.build variant "$@"
