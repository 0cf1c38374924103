set -o pipefail
for t in "random_sweep.py 200" "random_sweep_qact.py 150" "random_sweep_attn.py 60" "random_sweep_prefill_attn.py 120" "random_sweep_provider.py 60" "random_sweep_decoder.py 12" "random_sweep_qb32.py 80" "random_sweep_sampler.py 120" "random_sweep_sampler_chain.py 120" "random_sweep_mirostat.py 60" "random_sweep_constraints.py 200" "random_sweep_grammar.py 200" "random_sweep_extend.py 60" "random_sweep_fork.py 60" "random_sweep_shift.py 60" "random_sweep_logprob.py 150" "random_sweep_packed.py 40" "random_sweep_wide.py 24" "random_sweep_stop.py 300" "random_sweep_beam.py 24"; do
  echo "== $t"; timeout -k 10 500 python tools/$t 2>&1 | tail -n 2 || echo "FAILED $t"
done
