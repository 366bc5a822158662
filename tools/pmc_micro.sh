# Traffic of a micro-benchmark's kernels (tooling only): one FETCH_SIZE and one
# WRITE_SIZE pass, each a rocprofv3 run of its own with nothing traced beside
# the counter. The CSVs and traffic.jsonl go to $PMC_OUT (default: pmc_<binary>
# under the system's temporary directory).
# Usage: pmc_micro.sh <binary in bench/micro> <its argument> <kernel name substring> [...]
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); B=$1; A=$2; shift 2
O=${PMC_OUT:-${TMPDIR:-/tmp}/pmc_$B}; mkdir -p $O
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/fetch -o p -- $R/bench/micro/$B $A > $O/fetch.log 2>&1 && \
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/write -o p -- $R/bench/micro/$B $A > $O/write.log 2>&1 && \
python3 $R/tools/pmc_micro.py $O/fetch $O/write -- "$@" | tee $O/traffic.jsonl
echo "pmc_micro rc=$?"
