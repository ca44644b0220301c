# time prebuilt libgdeconv variants (variants/*.so) with the default bench
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${BENCH_OUT:-$R/bench_out}; mkdir -p $O
cp $R/galaxy-deconv_amd/gdeconv/libgdeconv.so /tmp/orig.so
for v in "$@"; do
  cp $R/variants/$v.so $R/galaxy-deconv_amd/gdeconv/libgdeconv.so
  timeout -k 10 200 python3 $R/bench.py --full --no-cpu-baseline --no-e2e --fused 1 > $O/var_$v.json 2> $O/var_$v.err || { echo "variant $v failed rc=$?"; break; }
  echo "variant $v done"
done
cp /tmp/orig.so $R/galaxy-deconv_amd/gdeconv/libgdeconv.so
